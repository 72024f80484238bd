#!/usr/bin/env python3
"""Headline benchmark: training samples/s (whole node) of DALL-E d_model=1024, 24 layers,
256 text + 32x32 image tokens, bf16 data-parallel on 1/2/4/8 MI355X (BASELINE.json config 2).

One process per GPU, RCCL over xGMI. ``python bench.py --gpus N`` either runs under a launcher that
already set ``WORLD_SIZE`` (torchrun: the driver's multi-GPU form) or, when it did not and N > 1,
starts the N worker processes itself (this script again, with torchrun's env contract) BEFORE any
GPU call in the parent. Every worker asserts that the process group really has N ranks.

Every timed step is a full training step: forward + backward (fused HIP kernels), gradient
all-reduce across ranks (bucketed, RCCL), global grad-norm clip and a LAMB optimizer update on
every parameter, i.e. a global step of the collaborative optimizer with ``target_batch_size`` equal
to the global batch. ``--engine collab`` times the collaborative optimizer's own ``.step()``
(``CollaborativeOptimizer``: accumulation, progress tracker, sample-weighted averaging, delayed
8-bit LAMB) -- the loop ``run_trainer.py`` drives -- and also reports its tracker's
``performance_ema`` (the reference's metric, ``callback.py:63``) summed over peers.

Data: synthetic LAION-shaped pairs (256 caption ids padded with 1, 1024 VQGAN codes), random-init
weights. Rank 0 prints ONE JSON line.

A plain run sets up, warms up, times ``--steps`` steps and prints that line. ``--dump-outputs DIR`` also writes
what the last timed step produced (``loss.npy``, ``params.npy``, ``grads.npy``; the inputs and the initial weights
are seeded, so two builds can be compared output for output). ``--full`` adds the measurements that need runs of
their own (world > 1: the gradient all-reduce alone, ``grad_allreduce.standalone_ms`` / ``busbw_GBps`` / ``buckets``).

CPU rehearsal: ``BENCH_BACKEND=gloo python bench.py --gpus 2 --model tiny --batch 2`` runs the same
path with gloo on CPU when no GPU is visible (tests/test_bench_cpu.py).
"""
from __future__ import annotations

import argparse
import json
import os
import socket
import subprocess
import sys
import time

import torch
import torch.distributed as dist

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from dalle_amd.config import get_config  # noqa: E402
from dalle_amd.data.synthetic import synthetic_batch  # noqa: E402
from dalle_amd.models.dalle import DALLE  # noqa: E402
from dalle_amd.optim import FlatArena, LAMB8bit  # noqa: E402
from dalle_amd.parallel.dp import GradSync  # noqa: E402

METRIC = "training samples/sec (whole node), DALL-E d_model=1024 at 1/2/4/8 MI355X"
MODEL_NAMES = {
    "bench24": "DALL-E d_model=1024, 24 layers, 256 text + 32x32 image tokens",
    "dalle-1024-24l": "DALL-E d_model=1024, 24 layers, 256 text + 32x32 image tokens",
    "dalle-1024-24l-unshared": "DALL-E d_model=1024, 24 layers (no weight sharing), 256 text + 32x32 image tokens",
    "reference": "DALL-E d_model=1024, 64 layers (5 shared blocks), reversible, 256 text + 32x32 image tokens",
    "dalle-1.3b": "DALL-E ~1.3B, reversible, 256 text + 32x32 image tokens",
    "tiny": "DALL-E tiny (2 layers, 64 text + 16x16 image tokens)",
}
BASELINE_VALUE = None  # the reference publishes no throughput numbers


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1, help="number of ranks (one per GPU)")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=int(os.environ.get("BENCH_BATCH", 128)),
                    help="per-GPU micro-batch (128: 187 GB of 288; with the token-contiguous weight-grad inputs B128 "
                         "beats B64 on the same box, 280.7/279.2/280.6 vs 275.1/276.8/275.8 samples/s, "
                         "profiles/r3s5_batch_ab.txt; earlier sweep: B48 259.7, B64 264.9, B80 258.5, B96 263.8, "
                         "B128 267.8, profiles/r3_batch_sweep.txt -- multiples of 64 keep every GEMM / attention grid a "
                         "whole number of waves)")
    ap.add_argument("--model", default="bench24")
    ap.add_argument("--engine", default="step", choices=["step", "collab"],
                    help="step: model + GradSync + fused LAMB; collab: the CollaborativeOptimizer.step() loop")
    ap.add_argument("--optim-bits", type=int, default=None, choices=[8, 32],
                    help="LAMB moment storage (default: 32 for --engine step, 8 = the reference's CPULAMB8Bit for collab)")
    ap.add_argument("--grad-dtype", default="fp32", choices=["fp32", "bf16"])
    ap.add_argument("--allreduce-algo", default=os.environ.get("DALLE_AMD_ALLREDUCE_ALGO", "auto"),
                    choices=["auto", "rccl", "rs_ag"],
                    help="gradient all-reduce: one RCCL all_reduce per bucket, or reduce-scatter + all-gather per bucket "
                         "(the explicit direct-mesh form, average fused into the reduce-scatter); auto (default): time "
                         "both at every --bucket-mb candidate on the real communicator at start-up and keep the fastest")
    ap.add_argument("--bucket-mb", default=os.environ.get("DALLE_AMD_BUCKET_MB", "auto"),
                    help="gradient bucket size in MB, or auto: 16/32/64/128 MB timed at start-up (with --allreduce-algo)")
    ap.add_argument("--compression", default="none", choices=["none", "powersgd", "uniform8bit"],
                    help="gradient averaging: plain bucketed all-reduce, PowerSGD rank-4 with error feedback "
                         "(BASELINE config 3) or the hivemind size-adaptive fp16 / uniform-8-bit butterfly")
    ap.add_argument("--powersgd-rank", type=int, default=4)
    ap.add_argument("--no-delay", action="store_true", help="collab engine: synchronous optimizer step")
    ap.add_argument("--profile-steps", type=int, default=0,
                    help="after the timed run: K more steps with per-phase timing (+ torch.profiler trace)")
    ap.add_argument("--trace", default="", help="chrome trace path for the --profile-steps pass")
    ap.add_argument("--no-recompute", action="store_true",
                    help="reversible presets: keep the activations instead of rebuilding them in backward")
    ap.add_argument("--recompute", default=None, choices=["true", "false", "auto"],
                    help="reversible presets: rebuild activations in backward (true, the reference regime), keep them "
                         "(false) or keep as many blocks as the free HBM holds (auto)")
    ap.add_argument("--tunable", default="off", choices=["auto", "use", "tune", "off"],
                    help="hipBLASLt solution selection for the library GEMMs (dalle_amd/utils/tuning.py)")
    ap.add_argument("--dump-outputs", default="", metavar="DIR",
                    help="after the timed steps, write what the last timed step produced as DIR/<name>.npy (float32): "
                         "loss, and a fixed seeded sample of the updated parameters and of the gradients it applied")
    ap.add_argument("--full", action="store_true",
                    help="also run the measurements that take runs of their own (world > 1: the gradient all-reduce "
                         "alone, whole and per bucket, for its standalone time and bus bandwidth); a plain run only "
                         "times the steps")
    return ap.parse_args()


# ------------------------------------------------------------------------------------------------
# launcher: N worker processes, started before the parent touches any GPU
# ------------------------------------------------------------------------------------------------
def _free_port() -> int:
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def visible_gpu_count():
    """GPUs this process may use, WITHOUT any HIP call (the launcher must not initialise the runtime):
    the *_VISIBLE_DEVICES lists if set, else the KFD topology's GPU nodes; None if unknown."""
    for var in ("HIP_VISIBLE_DEVICES", "ROCR_VISIBLE_DEVICES", "CUDA_VISIBLE_DEVICES"):
        v = os.environ.get(var)
        if v is not None:
            return len([x for x in v.split(",") if x.strip() != ""])
    root = "/sys/class/kfd/kfd/topology/nodes"
    try:
        n = 0
        for node in os.listdir(root):
            with open(os.path.join(root, node, "gpu_id")) as fh:
                n += int(fh.read().strip() or 0) != 0
        return n
    except OSError:
        return None


def spawn_workers(n: int) -> int:
    """Run this script as ``n`` ranks (RANK/LOCAL_RANK/WORLD_SIZE/MASTER_* like torchrun) and return
    the first non-zero exit code (the others are terminated), or 0. The parent never touches HIP: the
    device count comes from the environment / sysfs (visible_gpu_count)."""
    backend = os.environ.get("BENCH_BACKEND", "nccl")
    if backend == "nccl":
        ndev = visible_gpu_count()
        if ndev is not None and ndev < n:
            print(f"bench.py: --gpus {n} but only {ndev} GPU(s) are visible", file=sys.stderr)
            return 2
    port = _free_port()
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n),
                   GROUP_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env))
    rc = 0
    live = list(procs)
    while live:
        for p in list(live):
            code = p.poll()
            if code is None:
                continue
            live.remove(p)
            if code != 0 and rc == 0:
                rc = code
                for q in live:
                    q.terminate()
        time.sleep(0.05)
    for p in procs:
        p.wait()
    return rc


# ------------------------------------------------------------------------------------------------
# one rank
# ------------------------------------------------------------------------------------------------
def _param_groups(model):
    no_decay = ["bias", "LayerNorm.weight"]  # task.py:138-150 (only biases match dalle-pytorch names)
    named = list(model.named_parameters())
    return [
        {"params": [p for n, p in named if not any(nd in n for nd in no_decay)], "weight_decay": 0.045},
        {"params": [p for n, p in named if any(nd in n for nd in no_decay)], "weight_decay": 0.0},
    ]


def _lamb(groups, bits, arena=None):
    return LAMB8bit(groups, lr=0.0025, betas=(0.9, 0.96), eps=1e-6, weight_decay=0.045, clamp_value=10000.0,
                    max_grad_norm=4.0, reuse_grad_buffers=True, optim_bits=bits, arena=arena)


DUMP_SAMPLE = 1 << 22  # elements kept of each flat buffer: 16 MB of float32 per file


def dump_outputs(path, loss, arena) -> None:
    """What the last timed step handed back, as float32 ``.npy`` files: its loss, the parameters after its
    optimizer update and the gradient arena as that step left it (--engine step: the averaged gradients it
    applied). The flat buffers are sampled at fixed positions (seeded, sorted, the same for every run of the
    same model), so two builds compare element for element."""
    import numpy as np

    os.makedirs(path, exist_ok=True)
    if arena.numel > DUMP_SAMPLE:
        idx = torch.randint(arena.numel, (DUMP_SAMPLE,), generator=torch.Generator().manual_seed(4321)).sort().values
    else:
        idx = torch.arange(arena.numel)
    np.save(os.path.join(path, "loss.npy"), loss.detach().float().cpu().reshape(1).numpy())
    for name, buf in (("params", arena.data), ("grads", arena.grad)):
        np.save(os.path.join(path, f"{name}.npy"), buf.detach()[idx.to(buf.device)].float().cpu().numpy())


def run_rank(args) -> None:
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit(f"bench.py: --gpus {args.gpus} but the launcher started WORLD_SIZE={world} ranks")
    backend = os.environ.get("BENCH_BACKEND", "nccl")
    use_cuda = torch.cuda.is_available()
    if backend == "nccl" and not use_cuda:
        raise SystemExit("bench.py: no GPU visible (set BENCH_BACKEND=gloo for the CPU rehearsal)")
    if use_cuda:
        # one rank per GPU; more ranks than GPUs (a rehearsal of the multi-rank path on a 1-GPU box
        # with BENCH_BACKEND=gloo) share devices round-robin
        device = torch.device("cuda", local_rank % torch.cuda.device_count())
        torch.cuda.set_device(device)
    else:
        device = torch.device("cpu")
        torch.set_num_threads(max(1, min(4, (os.cpu_count() or 2) // max(1, world))))

    def sync():
        if use_cuda:
            torch.cuda.synchronize(device)

    if world > 1:
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=device)
        else:
            dist.init_process_group(backend)
        assert dist.get_world_size() == world, (dist.get_world_size(), world)
    torch.backends.cuda.matmul.allow_tf32 = False
    tuning = "off"
    if use_cuda:
        from dalle_amd.utils.tuning import setup_gemm_tuning
        tuning = setup_gemm_tuning(args.tunable if (args.tunable != "tune" or rank == 0) else "use")

    cfg = get_config(args.model)
    if args.no_recompute:
        cfg.reversible_recompute = False
    if args.recompute is not None:
        cfg.reversible_recompute = "auto" if args.recompute == "auto" else args.recompute == "true"
    bits = args.optim_bits if args.optim_bits is not None else (8 if args.engine == "collab" else 32)
    torch.manual_seed(1234)
    model = DALLE(cfg).to(device)
    arena = FlatArena(model.parameters(), device=device)
    model.grad_arena = arena
    if world > 1:  # identical init on every rank
        dist.broadcast(arena.data, 0)
    groups = _param_groups(model)
    named = list(model.named_parameters())
    pg = dist.group.WORLD if world > 1 else None

    gen = torch.Generator().manual_seed(1000 + rank)
    batches = [synthetic_batch(args.batch, cfg.text_seq_len, cfg.image_seq_len, cfg.num_text_tokens,
                               cfg.num_image_tokens, gen, device=device) for _ in range(4)]
    if args.engine == "collab":
        from dalle_amd.parallel.compression import reference_averaging_compression, NoCompression
        from dalle_amd.parallel.optimizer import CollaborativeOptimizer
        comp = reference_averaging_compression() if args.compression == "uniform8bit" else NoCompression()
        copt = CollaborativeOptimizer(
            dht=None, run_id="bench", params=groups, optimizer=lambda g: _lamb(g, bits),
            target_batch_size=args.batch * world, batch_size_per_step=args.batch,
            offload_optimizer=True, delay_optimizer_step=not args.no_delay, reuse_grad_buffers=True,
            grad_compression=comp, state_averaging_compression=comp, process_group=pg, arena=arena,
            powersgd_rank=args.powersgd_rank if args.compression == "powersgd" else None,
            tracker_mode="static", device=device)

        def opt_step():
            copt.step()
        zero = None  # the collaborative optimizer resets the accumulated grads after each global step
    else:
        opt = _lamb(groups, bits, arena=arena)
        ar_tuning = None
        algo = args.allreduce_algo
        bucket_bytes = None if args.bucket_mb == "auto" else int(float(args.bucket_mb) * 2 ** 20)
        if world > 1 and args.compression == "none" and (algo == "auto" or bucket_bytes is None):
            # pick the all-reduce form for THIS mesh (xGMI point-to-point links, or gloo in the CPU rehearsal):
            # every candidate timed over the real arena, max over ranks, so every rank selects the same one
            from dalle_amd.parallel.dp import tune_grad_sync
            algos = ("rccl", "rs_ag") if algo == "auto" else (algo,)
            mbs = (16, 32, 64, 128) if bucket_bytes is None else (bucket_bytes / 2 ** 20,)

            def tune_step(gs):
                # the candidate inside a real step: zero, forward, backward (final grads handed to gs as they
                # appear when overlapped), the remaining all-reduce -- no optimizer step, params untouched
                arena.zero_grad()
                b = batches[0]
                model(b["input_ids"], b["image"], mask=b["attention_mask"], return_loss=True).backward()
                gs.all_reduce()

            algo, bucket_bytes, ar_tuning = tune_grad_sync(
                arena, world, grad_dtype=args.grad_dtype, algos=algos, bucket_mb=mbs, step_fn=tune_step,
                overlap=os.environ.get("DALLE_AMD_DP_OVERLAP", "1") != "0")
        if algo == "auto":
            algo = "rccl"
        if bucket_bytes is None:
            from dalle_amd.parallel.dp import DEFAULT_BUCKET_BYTES
            bucket_bytes = DEFAULT_BUCKET_BYTES
        args.allreduce_algo = algo
        sync_grads = GradSync(arena, world_size=world, grad_dtype=args.grad_dtype, algo=algo, bucket_bytes=bucket_bytes)
        if args.compression == "powersgd":
            # compression work runs at every world size (the all-reduces are skipped only when world == 1)
            from dalle_amd.parallel.powersgd import PowerSGD
            psgd = PowerSGD([p for _, p in named], rank=args.powersgd_rank, seed=0)
            reduce_grads = psgd.allreduce_
        elif args.compression == "uniform8bit":
            from dalle_amd.parallel.averaging import allreduce_weighted
            from dalle_amd.parallel.compression import reference_averaging_compression
            comp = reference_averaging_compression()

            def reduce_grads():
                allreduce_weighted(arena.grad, 1.0, compression=comp, segments=arena.segments())  # no-op on one GPU
        else:
            reduce_grads = sync_grads.all_reduce
            if os.environ.get("DALLE_AMD_DP_OVERLAP", "1") != "0":
                sync_grads.attach()  # all-reduce grads that are final while the rest of backward runs

        def opt_step():
            reduce_grads()
            opt.step()
        zero = arena.zero_grad


    from dalle_amd.utils.profiling import StepTimer, prof_range

    def step(i, timer=None):
        phase = timer if timer is not None else (lambda name: prof_range(name))
        b = batches[i % len(batches)]
        if zero is not None:
            zero()
        with phase("forward"):
            loss = model(b["input_ids"], b["image"], mask=b["attention_mask"], return_loss=True)
        with phase("backward"):
            loss.backward()
        with phase("grad_averaging+optimizer"):
            opt_step()
        return loss

    for i in range(args.warmup):
        loss = step(i)
    sync()
    if world > 1:
        dist.barrier()
    sync()
    comm = sync_grads if (args.engine == "step" and world > 1 and args.compression == "none") else None
    if comm is not None:
        comm.reset_stats()
        comm.timing = use_cuda
    if use_cuda:
        torch.cuda.reset_peak_memory_stats(device)
    t0 = time.perf_counter()
    for i in range(args.steps):
        loss = step(i)
    sync()
    if world > 1:
        dist.barrier()
    sync()
    elapsed = time.perf_counter() - t0
    if args.engine == "collab":
        copt.apply_pending()
    if args.dump_outputs and rank == 0:  # every rank holds the same parameters and averaged gradients
        dump_outputs(args.dump_outputs, loss, arena)
    per_rank = [elapsed]
    names = [torch.cuda.get_device_name(device) if use_cuda else "cpu"]
    if world > 1:
        per_rank = [None] * world
        names_all = [None] * world
        dist.all_gather_object(per_rank, elapsed)
        dist.all_gather_object(names_all, names[0])
        names = names_all
    elapsed = max(per_rank)
    final_loss = float(loss.item())
    peak_gb = round(torch.cuda.max_memory_allocated(device) / 2 ** 30, 2) if use_cuda else None
    comm_stats = None
    if comm is not None:
        comm.timing = False
        exposed = comm.exposed_ms() / args.steps if use_cuda else None
        step_bytes = comm.bytes_reduced / args.steps
        overlapped = round(comm.last_early_elems / max(1, arena.numel), 3)
        t_ar = None
        if args.full:
            # the same all-reduce (same buckets) alone, to price the bytes: bus bandwidth as nccl-tests reports it
            g = arena.grad
            saved = g.clone()
            sync()
            dist.barrier()
            ta = time.perf_counter()
            for _ in range(3):
                comm.all_reduce()
            sync()
            t_ar = (time.perf_counter() - ta) / 3
            g.copy_(saved)
            del saved
            t_all = [None] * world
            dist.all_gather_object(t_all, t_ar)
            t_ar = max(t_all)
        comm_stats = {"algo": args.allreduce_algo, "buckets": comm.bucket_busbw() if args.full else None,
                      "selected": {"algo": args.allreduce_algo, "bucket_mb": round(comm.bucket_elems * 4 / 2 ** 20, 1),
                                   "tuned": ar_tuning is not None},
                      "tuning": ar_tuning,
                      "bytes_per_step": int(step_bytes),
                      "standalone_ms": None if t_ar is None else round(t_ar * 1e3, 3),
                      "busbw_GBps": None if t_ar is None else round(2 * (world - 1) / world * step_bytes / t_ar / 1e9, 1),
                      "exposed_ms_per_step": None if exposed is None else round(exposed, 3),
                      "overlapped_frac": overlapped}
    peaks = [peak_gb]
    if world > 1:
        peaks = [None] * world
        dist.all_gather_object(peaks, peak_gb)
    ema = None
    if args.engine == "collab":
        mine = copt.tracker.performance_ema.flush()  # every recorded step's device interval folded in
        sps = [mine]
        if world > 1:
            sps = [None] * world
            dist.all_gather_object(sps, mine)
        ema = sum(sps)

    samples = args.batch * world * args.steps
    value = samples / elapsed
    ms = elapsed / args.steps * 1000
    if rank == 0:
        tflops = cfg.train_flops_per_sample() * value / world / 1e12  # model FLOPs (no recompute)
        hw_tflops = cfg.train_flops_per_sample(include_recompute=True) * value / world / 1e12
        n_attn = len(set(map(str, cfg.shared_attn_ids)))
        n_ff = len(set(map(str, cfg.shared_ff_ids)))
        sharing = (f"{n_attn} unique attn / {n_ff} unique ff blocks over {cfg.depth} layers"
                   if (n_attn < cfg.depth or n_ff < cfg.depth) else "none")
        out = {
            "metric": METRIC,
            "value": round(value, 3),
            "unit": "samples/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(ms, 3),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None if BASELINE_VALUE is None else value / BASELINE_VALUE,
            "dtype": "bf16" if use_cuda else "fp32",
            "data": "synthetic LAION-shaped pairs (256 caption ids + 32x32 VQGAN codes), random-init weights",
            "config": {"model": MODEL_NAMES.get(args.model, args.model),
                       "preset": args.model, "global_batch": args.batch * world, "per_gpu_batch": args.batch,
                       "seq_len": cfg.seq_len, "parallelism": f"dp{world}",
                       "weight_sharing": sharing,
                       "unique_params": cfg.unique_param_count(),
                       "engine": "CollaborativeOptimizer.step" if args.engine == "collab" else "GradSync + fused LAMB",
                       "optimizer": f"LAMB ({bits}-bit moments) + global clip 4.0",
                       "grad_allreduce_dtype": args.grad_dtype, "grad_allreduce_algo": args.allreduce_algo,
                       "gemm_selection": tuning,
                       "reversible": ({True: "recompute", False: "stored activations"}.get(cfg.reversible_recompute, "auto: stored while HBM allows")
                                      if cfg.reversible else "no"),
                       "grad_compression": args.compression if args.compression != "powersgd"
                       else f"powersgd-rank{args.powersgd_rank}"},
            "rccl_world": world if backend == "nccl" else None,
            "backend": backend if world > 1 else "none",
            "devices": names,
            "per_rank_ms_per_step": [round(t / args.steps * 1000, 3) for t in per_rank],
            "model_tflops_per_gpu": round(tflops, 1),
            "hw_tflops_per_gpu": round(hw_tflops, 1),
            "max_mem_gb": round(torch.cuda.max_memory_allocated(device) / 2 ** 30, 1) if use_cuda else None,
            "loss": round(final_loss, 4),
        }
        if ema is not None:
            out["collab_performance_ema_samples_per_s"] = round(ema, 3)
            out["collab_ema_over_wall"] = round(ema / value, 4)
            out["collab_backward_overlapped_rounds"] = copt.grad_averager.overlapped_rounds
            if use_cuda and args.steps >= 5 and abs(ema / value - 1.0) > 0.03:
                # the reference's metric (callback.py:63) must report what the wall clock sees
                raise SystemExit(f"performance_ema {ema:.2f} samples/s deviates > 3 % from the wall clock {value:.2f}")
        out["per_rank_peak_mem_gb"] = peaks
        if comm_stats is not None:
            out["grad_allreduce"] = comm_stats
            out["grad_allreduce_overlapped_frac"] = comm_stats["overlapped_frac"]
        if os.environ.get("BENCH_DUMP_PARAMS"):
            out["param_checksum"] = float(arena.data.double().sum())
        print(json.dumps(out), flush=True)
    if os.environ.get("BENCH_DUMP_PARAMS"):
        torch.save(arena.data.detach().cpu(), f"{os.environ['BENCH_DUMP_PARAMS']}.rank{rank}.pt")
    if args.profile_steps:
        # untimed diagnostic pass: per-phase wall times (synchronised) and an optional trace
        timer = StepTimer()
        prof = None
        if args.trace:
            prof = torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CPU,
                                                      torch.profiler.ProfilerActivity.CUDA])
            prof.__enter__()
        for i in range(args.profile_steps):
            step(i, timer)
        if prof is not None:
            prof.__exit__(None, None, None)
            if rank == 0:
                prof.export_chrome_trace(args.trace)
        if rank == 0:
            print("# phase ms/step: " + json.dumps(timer.summary()), file=sys.stderr, flush=True)
    if world > 1:
        dist.destroy_process_group()


def main() -> int:
    args = parse()
    if args.gpus < 1:
        raise SystemExit("--gpus must be >= 1")
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        return spawn_workers(args.gpus)
    run_rank(args)
    return 0


if __name__ == "__main__":
    sys.exit(main())
