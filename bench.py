#!/usr/bin/env python3
"""Headline benchmark: mclSTExp contrastive TRAINING STEP throughput on MI355X.

    python bench.py [--gpus N --steps K --warmup W]          # N > 1: this process spawns N workers itself
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
        --master-port P bench.py --gpus N --steps K --warmup W

One step = train.py:33-41 of the reference on one synthetic batch already resident in HBM:
DenseNet-121 image encoder -> ProjectionHead, position-embedding add -> 2-layer spot Transformer ->
ProjectionHead, B x B logits + symmetric InfoNCE, backward, Adam(lr 1e-4, wd 1e-3) over ALL
parameters including both (65536, G) position tables.  Workload = BASELINE.json configs[1]:
batch 128 per GPU, 224x224 patches, 1000 genes, bf16 backbone.  N > 1 = data parallel, per-GPU batch
fixed (weak scaling), global InfoNCE over the all-gathered embeddings.

Prints ONE JSON line (rank 0).  `value` = spots/s of the whole job = steps/s x global batch.  A plain run does only
what that figure needs: set-up, the W warm-up steps, the K timed steps, the dump below if asked for, the line.

`--full` adds, after the timed region, what the headline does not need:
`roofline` = the C-ABI launch unit with the LARGEST time per step (`roofline_kernels` lists the others), each
call timed with HIP events on its launch stream in an eager pass right after the timed region (same process, same
resident model and inputs; every kernel alone on the GPU: side streams off), with the step's kernel audit
(`config.step_kernel_audit`).  `config.position_tables` = the cost of materialising the lazy position tables.
`config.parity_at_benched_shape` = the parity figures the GPU tests recorded.  `cpu_baseline` = the CPU oracle
(oracle/ref_cpu.py) timed on this host's cores on the same workload, a bounded number of steps (N=1 only).
`--no_cpu_baseline` and `--profile_steps 0` leave parts of that out.

`--dump-outputs DIR` writes what the last timed step computed as DIR/<name>.npy (``dump_outputs``).  The inputs and the
model's initial state are seeded, so two builds run with the same arguments can be compared array for array.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

# Kernel arguments in device memory (the image's default; measured here: 13.4 ms/step, 14.4 with =0).  Read when the HIP
# runtime library is loaded, i.e. it must be in the environment before torch is imported.
os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402   (importing torch does not initialise the GPU)

HBM_PEAK_GBS = 8000.0           # /opt/skills/guides/MI355X_MICROARCH.md: HBM3E ~8 TB/s
MFMA_BF16_PEAK_TFS = 2500.0     # same guide: dense bf16 MFMA peak
MALL_BYTES = 256e6              # Infinity Cache: a launch whose working set is smaller never needs HBM


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--batch", type=int, default=128, help="per-GPU batch (BASELINE configs[1]: 128)")
    ap.add_argument("--genes", type=int, default=1000)
    ap.add_argument("--image", type=int, default=224)
    ap.add_argument("--n_batches", type=int, default=16, help="distinct synthetic batches resident in HBM, cycled")
    ap.add_argument("--encoder", type=str, default="densenet121")
    ap.add_argument("--image_dim", type=int, default=1024)
    ap.add_argument("--compute", type=str, default="f32", choices=["f32", "bf16"],
                    help="MFMA operand type of the hand-written spot-path kernels")
    ap.add_argument("--infonce", type=str, default="fused", choices=["fused", "exact", "fp8"],
                    help="fused = flash-style bf16 MFMA InfoNCE (logits never in HBM); exact = fp32 GEMM + LSE kernels; "
                         "fp8 = the fused kernel on e4m3 operands (BASELINE configs[4])")
    ap.add_argument("--backbone_dtype", type=str, default="bf16", choices=["bf16", "f32"])
    ap.add_argument("--full", action="store_true",
                    help="after the timed region also time the kernels one by one (`roofline`, kernel audit), the position "
                         "tables' materialisation and the CPU oracle (`cpu_baseline`), and relay the recorded parity figures")
    ap.add_argument("--no_cpu_baseline", action="store_true", help="with --full: no `cpu_baseline`")
    ap.add_argument("--no_graphs", action="store_true", help="A/B: eager launches instead of HIP-graph replay")
    ap.add_argument("--unfused_backbone", action="store_true", help="A/B: plain torch module path for the backbone")
    ap.add_argument("--cpu_budget_s", type=float, default=25.0)
    ap.add_argument("--profile_steps", type=int, default=2,
                    help="with --full: eager steps after the timed region in which the hot C-ABI calls are timed with HIP "
                         "events (0 = no `roofline` object)")
    ap.add_argument("--dense_tables", action="store_true",
                    help="A/B: update every row of the two position tables on every step (1.57 GB of state traffic) instead of "
                         "the lazy-exact form (optim.FusedAdam(lazy_tables=True): untouched rows are replayed on demand)")
    ap.add_argument("--serial_lanes", action="store_true",
                    help="profiling aid: no side streams (every kernel alone on the GPU, one lane) -- the schedule the serial "
                         "rocprofv3 traces under profiles/ record; results are bit-identical to the two-lane step")
    ap.add_argument("--launch_check", action="store_true",
                    help="only exercise the launcher + process group (works without a GPU, gloo): prints a JSON line")
    ap.add_argument("--dump-outputs", dest="dump_outputs", type=str, default=None, metavar="DIR",
                    help="after the timed steps, write what the last timed step computed (loss, embeddings, parameters, "
                         "gradients, BatchNorm statistics) as DIR/<name>.npy (rank 0; see dump_outputs)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    if args.warmup < 0:
        ap.error("--warmup must not be negative")
    return args


def _host_cores() -> int:
    try:
        return max(1, len(os.sched_getaffinity(0)))
    except AttributeError:
        return os.cpu_count() or 1


def _cpu_baseline_worker(genes: int, image: int, batch: int, budget_s: float) -> dict:
    """Runs in a child process (no GPU init): the CPU oracle's full training step on the host cores, at the GPU
    workload's own batch size."""
    from mclstexp_amd import synth
    from mclstexp_amd.backbones import densenet121_features_module
    from oracle import ref_cpu
    # Thread count: measured on the MI355X host (256 hardware threads), this step takes 2.0 s at 32 threads,
    # 10 s at 128 and does not finish in 5 min at 256 (oneDNN/OpenMP oversubscription) -> cap at 32.
    cores = min(32, _host_cores())
    torch.set_num_threads(cores)
    G = genes
    torch.manual_seed(0)
    params = synth.make_params(G, 1024, seed=0)
    net = densenet121_features_module()
    for k, v in net.state_dict().items():
        if v.dtype == torch.float32 and "running_" not in k:
            params["image_encoder.model.0." + k] = v.clone()
    for p in params.values():
        p.requires_grad_(True)
    state = {}
    b = synth.make_batch(batch, G, image_hw=image, seed=0)
    ref_cpu.train_step(params, state, b, 1)               # warm-up (allocations, oneDNN primitives)
    n_steps, t0 = 0, time.perf_counter()
    while n_steps < 6 and (n_steps < 2 or time.perf_counter() - t0 < budget_s):
        ref_cpu.train_step(params, state, b, n_steps + 2)
        n_steps += 1
    t = (time.perf_counter() - t0) / n_steps
    return {"value": round(batch / t, 3), "unit": "spots/s", "cores": cores, "kind": "port",
            "steps_per_sec": round(1.0 / t, 4),
            "sample": f"oracle/ref_cpu.train_step (fp32 torch CPU: DenseNet-121 restatement + spot path + dense-table "
                      f"Adam over all params), batch {batch} x {image}^2 patches x {G} genes = the GPU workload, "
                      f"1 warm-up + {n_steps} timed steps, {t:.2f} s/step, {cores} threads"}


def cpu_baseline(args, budget_s: float):
    """Oracle (a port: the reference cannot run unmodified on CPU) timed on the host cores in a
    child process with a hard wall-clock limit, so a --full run always finishes."""
    import subprocess
    code = ("import json,sys; sys.path.insert(0, %r); import bench; "
            "print('CPUBASE ' + json.dumps(bench._cpu_baseline_worker(%d, %d, %d, %f)))"
            % (ROOT, args.genes, args.image, args.batch, budget_s))
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="")
    limit = max(120.0, 8 * budget_s)
    try:
        r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=limit, env=env)
        for line in r.stdout.splitlines():
            if line.startswith("CPUBASE "):
                return json.loads(line[8:])
        return {"value": None, "unit": "spots/s", "cores": _host_cores(), "kind": "port",
                "sample": "cpu baseline failed: " + (r.stderr.strip().splitlines() or ["?"])[-1][:200]}
    except subprocess.TimeoutExpired:
        return {"value": None, "unit": "spots/s", "cores": _host_cores(), "kind": "port",
                "sample": f"cpu baseline exceeded its {limit:.0f} s wall-clock limit"}


_RESULT_FD = 1


def log(msg: str) -> None:
    if int(os.environ.get("RANK", "0")) == 0:
        print(f"[bench {time.strftime('%H:%M:%S')}] {msg}", file=sys.stderr, flush=True)


# ------------------------------------------------------------------------------------------------ kernel roofline
# C-ABI launch unit -> (kernels it enqueues, bound, algorithmic bytes of ONE call from its argument tuple).
# Algorithmic bytes = every operand element read once + every result element written once.
def _kernel_table():
    from mclstexp_amd import kernel_costs
    return kernel_costs.TABLE


def baseline_config_name(args):
    """Which BASELINE.json config the flags describe (the default flags = configs[1], the metric's own config)."""
    key = (args.encoder, args.batch, args.image, args.genes)
    if key == ("densenet121", 128, 224, 1000):
        return "BASELINE configs[1]"
    if key == ("densenet121", 8, 112, 785):
        return "BASELINE configs[0]"
    if args.encoder in ("vit", "vit_b16") and args.batch == 256:
        return "BASELINE configs[2] (%s)" % ("ViT-B/32" if args.encoder == "vit" else "ViT-B/16")
    if key == ("densenet121", 256, 256, 3467):
        return "BASELINE configs[4] per-GPU shape"
    return "non-BASELINE configuration"


def parity_artifact(args):
    """Parity figures of the benched mode are MEASURED by tests/test_configs_gpu.py::test_cfg1_as_benched_vs_oracle and the
    per-layer tests; the test run writes them to profiles/parity_at_benched_shape.json with the commit they were taken at.
    This line only relays that artifact (nothing is re-measured here, no constants live in this file)."""
    if baseline_config_name(args) != "BASELINE configs[1]":
        return None
    path = os.path.join(ROOT, "profiles", "parity_at_benched_shape.json")
    try:
        with open(path) as f:
            d = json.load(f)
        d["source"] = "profiles/parity_at_benched_shape.json (written by the GPU test run named inside; not re-measured by bench.py)"
        return d
    except Exception:
        return {"source": "tests/test_configs_gpu.py::test_cfg1_as_benched_vs_oracle, tests/test_layerwise_gpu.py (no artifact found)"}


def kernel_roofline(step_fn, n_steps: int, model) -> list:
    """Eager pass: every listed C-ABI call of ``n_steps`` steps is bracketed by HIP events on its launch stream.
    Side streams are switched off for the pass so that each timed launch has the GPU to itself (the durations are
    then comparable with the serial rocprofv3 kernel trace under profiles/)."""
    from mclstexp_amd import _lib, densenet_fused as dn
    table = _kernel_table()
    side, overlap = dn.USE_SIDE_STREAM, type(model).overlap_branches
    dn.USE_SIDE_STREAM, type(model).overlap_branches = False, False
    try:
        step_fn(0)                                        # un-timed: first eager call after graph replay
        torch.cuda.synchronize()
        with _lib.AbiTimer(list(table)) as t:
            for i in range(n_steps):
                step_fn(i + 1)
            summ = t.summary()
    finally:
        dn.USE_SIDE_STREAM, type(model).overlap_branches = side, overlap
    traffic, traffic_meta = {}, None
    tpath = os.path.join(ROOT, "profiles", "kernel_traffic.json")
    if os.path.exists(tpath):
        try:
            traffic = json.load(open(tpath))
            traffic_meta = traffic.pop("_source", None) or (
                "profiles/kernel_traffic.json: rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of this command in an earlier "
                "run (FETCH doubled per the gfx950 correction), NOT measured in this run")
        except Exception:
            traffic = {}
    rows = []
    # entry points that are the same launch unit (kernel_costs "unit": e.g. mcl_dense_conv3x3_bwd_fix = mcl_dense_conv3x3_bwd
    # with the folded bn1_fix on the 14 x 14 / 7 x 7 layers) are merged into one row, each call priced by its own formula
    units = {}
    for name, s in summ.items():
        spec = table[name]
        u = units.setdefault(spec.get("unit") or name, {"calls": 0, "total_ms": 0.0, "alg": [], "strict": [], "flops": []})
        u["calls"] += s["calls"]
        u["total_ms"] += s["total_ms"]
        u["alg"] += [float(spec["bytes"](a)) for a in s["args"]]
        u["strict"] += [float(spec["strict"](a)) for a in s["args"]]
        u["flops"] += [float(spec["flops"](a)) for a in s["args"]]
    for name, u in units.items():
        spec = table[name]
        s = {"calls": u["calls"], "total_ms": u["total_ms"], "avg_ms": u["total_ms"] / u["calls"]}
        alg, strict, flops = u["alg"], u["strict"], u["flops"]
        tot_b, tot_strict, tot_s = sum(alg), sum(strict), s["total_ms"] * 1e-3
        # `achieved` / `frac`: STRICT algorithmic bytes (every distinct operand / result element once, whatever the unit's
        # internal passes) over the measured time; the as-built figure (a tensor handed between the unit's own kernels through
        # HBM counted written and re-read) is kept beside it as `frac_as_built`
        ach = tot_strict / tot_s / 1e9
        ach_built = tot_b / tot_s / 1e9
        tfs = sum(flops) / tot_s / 1e12
        tr = traffic.get(name)
        # which roofline bounds the unit: the 3x3 family is MFMA / LDS paced; a unit whose launches are short AND whose
        # working set fits the Infinity Cache is latency-bound (an HBM roofline is not the operative bound there)
        bound = spec["bound"]
        if bound is None:
            bound = "latency" if (max(strict) < MALL_BYTES and s["avg_ms"] < 0.030) else "hbm"
        rows.append({"abi": name, "kernel": spec["kernels"], "bound": bound, "achieved": round(ach, 1),
                     "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(ach / HBM_PEAK_GBS, 4),
                     "traffic": tr,
                     "traffic_source": traffic_meta,
                     "launches_per_step": s["calls"] / n_steps,
                     "avg_launch_ms": round(s["avg_ms"], 5), "ms_per_step": round(s["total_ms"] / n_steps, 4),
                     "algorithmic_bytes": round(tot_strict / s["calls"], 1),
                     "algorithmic_bytes_as_built": round(tot_b / s["calls"], 1),
                     "frac_as_built": round(ach_built / HBM_PEAK_GBS, 4),
                     "strict_bytes_per_step": round(tot_strict / n_steps, 1),
                     "flops": round(sum(flops) / s["calls"], 1), "tflops": round(tfs, 1),
                     "mfma_frac": round(tfs / MFMA_BF16_PEAK_TFS, 4)})
    rows.sort(key=lambda r: -r["ms_per_step"])
    return rows


# ------------------------------------------------------------------------------------------------ output dump
DUMP_SAMPLE = 32768            # elements kept per tensor: all of a smaller one, a fixed seeded sample of a larger one
DUMP_LIMIT_BYTES = 64 << 20


def _dump_sample(t):
    """fp32 host copy of ``t`` flattened; above DUMP_SAMPLE elements only the positions drawn by a generator seeded with 0
    (sorted), so two runs -- or two builds -- sample the same elements of a tensor of the same size."""
    import numpy as np
    f = t.detach().reshape(-1)
    if f.numel() > DUMP_SAMPLE:
        idx = np.sort(np.random.default_rng(0).choice(f.numel(), DUMP_SAMPLE, replace=False))
        f = f[torch.from_numpy(idx).to(f.device)]
    return f.float().cpu().numpy()


def dump_outputs(out_dir: str, loss, trainer, model) -> dict:
    """What the timed path hands its caller after its last step, as ``out_dir/<name>.npy``:
      loss                       float64 (1,)
      spot_embedding, image_embedding   fp32 (B, 256) of the last step (graph replay only: the captured output buffers)
      param.<name>, grad.<name>, buffer.<name>   fp32, flattened (sampled above DUMP_SAMPLE elements): the parameters the
                                 step's optimizer update left (position tables materialised), their gradients of the last
                                 step, the BatchNorm running statistics
    Called outside the timed region, before anything else runs a step."""
    import numpy as np
    arrays = {"loss": np.array([float(loss)], dtype=np.float64)}
    if trainer.graphs and trainer.es is not None and trainer.ei is not None:
        arrays["spot_embedding"] = trainer.es.detach().float().cpu().numpy()
        arrays["image_embedding"] = trainer.ei.detach().float().cpu().numpy()
    for n, p in model.named_parameters():
        arrays["param." + n] = _dump_sample(p)
        if p.grad is not None:
            arrays["grad." + n] = _dump_sample(p.grad)
    for n, b in model.named_buffers():
        if b.is_floating_point():
            arrays["buffer." + n] = _dump_sample(b)
    total = sum(a.nbytes for a in arrays.values())
    if total > DUMP_LIMIT_BYTES:
        raise RuntimeError(f"--dump-outputs: {total} bytes exceed the {DUMP_LIMIT_BYTES}-byte limit")
    os.makedirs(out_dir, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"), a)
    return {"dir": out_dir, "arrays": len(arrays), "bytes": total}


# ------------------------------------------------------------------------------------------------ launcher
def launch_check() -> None:
    """Launcher / rendezvous self-test (no GPU needed): every rank contributes rank+1 to an all-reduce."""
    from mclstexp_amd import dist as mdist
    os.environ.setdefault("MCL_DIST_BACKEND", "gloo" if not torch.cuda.is_available() else "nccl")
    pg, rank, world = mdist.init_from_env()
    t = torch.tensor([float(rank + 1)])
    if pg is not None:
        if torch.cuda.is_available() and os.environ["MCL_DIST_BACKEND"] == "nccl":
            t = t.cuda()
        torch.distributed.all_reduce(t, group=pg)
    if rank == 0:
        print(json.dumps({"launch_check": True, "world": world, "sum": float(t.item())}), flush=True)
    mdist.shutdown()


def main():
    args = parse()
    from mclstexp_amd import launch
    if args.gpus > 1 and not launch.under_launcher():
        # parent: no GPU call has been made (torch.cuda is untouched) -> start one fresh worker per GPU and relay
        # rank 0's JSON line.  Never re-exec a process that has initialised HIP.
        raise SystemExit(launch.spawn_workers(os.path.abspath(__file__), sys.argv[1:], args.gpus))
    world_env = int(os.environ.get("WORLD_SIZE", "1"))
    if world_env != args.gpus and not (args.gpus == 1 and world_env == 1):
        raise SystemExit(f"bench.py: --gpus {args.gpus} but the launcher started WORLD_SIZE={world_env} ranks")
    if args.launch_check:
        return launch_check()

    # stdout carries exactly ONE line, the JSON result: libraries that print from C (RCCL's version banner at
    # communicator creation) are pointed at stderr for the whole run; the result goes out through the saved descriptor
    global _RESULT_FD
    sys.stdout.flush()
    _RESULT_FD = os.dup(1)
    os.dup2(2, 1)
    from mclstexp_amd import dist as mdist
    pg, rank, world = mdist.init_from_env()
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X (the hot path has no CPU fallback)")
    dev = torch.device("cuda", torch.cuda.current_device())
    from mclstexp_amd import _lib, synth
    from mclstexp_amd.model import mclSTExp_Attention
    from mclstexp_amd.optim import FusedAdam
    _lib.lib()

    torch.manual_seed(0)
    bb = torch.bfloat16 if args.backbone_dtype == "bf16" else None
    model = mclSTExp_Attention(args.encoder, 1.0, args.image_dim, args.genes, 256, 8, 64, 2, compute=args.compute,
                               backbone_dtype=bb, embedding_grad="rowsparse",
                               process_group=pg, infonce=args.infonce)
    from mclstexp_amd import densenet_fused
    if args.serial_lanes:
        densenet_fused.USE_SIDE_STREAM = False
        type(model).overlap_branches = False
    model.fused_backbone = not args.unfused_backbone
    model.to(dev)
    if bb is not None:
        model.to(memory_format=torch.channels_last)
    model.train()
    opt = FusedAdam(model.parameters(), lr=1e-4, weight_decay=1e-3, lazy_tables=not args.dense_tables).attach_model(model)
    dist_on = pg is not None            # world > 1, or MCL_FORCE_DIST=1 (size-1 RCCL group: DP code path on one GPU)
    reducer = mdist.GradReducer(pg) if dist_on else None

    # synthetic inputs, resident in HBM before the timed region: args.n_batches distinct batches, cycled (expression /
    # position from the procedural formula; pixels uniform[0,1) from a seeded device generator -- 19 M values per batch)
    batches = []
    gen = torch.Generator(device=dev)
    for s in range(args.n_batches):
        b = synth.make_batch(args.batch, args.genes, seed=s, rank=rank)
        gen.manual_seed(1234 + 1000 * rank + s)
        b["image"] = torch.rand((args.batch, 3, args.image, args.image), device=dev, generator=gen)
        b = {k: v.to(dev) for k, v in b.items()}
        if bb is not None:
            b["image"] = b["image"].contiguous(memory_format=torch.channels_last)
        batches.append(b)

    from mclstexp_amd.engine import TrainStep
    # synthetic batches: every rank sees the same per-rank size on every step -> no per-step host size exchange
    trainer = TrainStep(model, opt, reducer, graphs=not args.no_graphs, warmup=3, equal_shards=True)

    def step(i):
        return trainer(batches[i % len(batches)])

    # setup (not part of the W warm-up steps): flat optimizer bucket, HIP-graph capture
    log("setup: 3 eager steps + graph capture")
    for i in range(5 if not args.no_graphs else 2):
        step(i)
    torch.cuda.synchronize()
    densenet_fused.reset_fallbacks()        # (the very first eager step precedes FusedAdam's flat gradient bucket)
    log(f"model + inputs resident; warm-up {args.warmup} steps")
    for i in range(args.warmup):
        loss = step(i)
    torch.cuda.synchronize()
    log("timed region")
    if dist_on:
        torch.distributed.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    n_host = min(8, args.steps)
    for i in range(args.steps):
        loss = step(i)
        if i + 1 == n_host:
            t_host = (time.perf_counter() - t0) / n_host      # host enqueue time per step, before queue back-pressure
    torch.cuda.synchronize()
    if dist_on:
        torch.distributed.barrier()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    log(f"host enqueue {1e3 * t_host:.2f} ms/step (first {n_host} steps), wall {1e3 * dt / args.steps:.2f} ms/step "
        f"({'HOST-bound' if t_host > 0.9 * dt / args.steps else 'GPU-bound'})")
    final_loss_t = loss.detach()
    final_loss = float(loss.item())
    if dist_on:
        t = torch.tensor([dt], device=dev, dtype=torch.float64)
        torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
        dt = float(t.item())

    # Lazy-exact position tables: the rows no batch touched are advanced when the table is materialised (state_dict /
    # checkpoint).  That work is deferred, not skipped -- with --full, time a full materialisation now (every row replays all
    # the steps of this run) and report it separately and amortised over the steps it covers.  The dump below holds the
    # materialised tables, so --dump-outputs materialises them too.
    tables_info = {"mode": "dense: every row of both tables on every step"}
    if opt.lazy_tables and opt._tables:
        tables_info = {"mode": "lazy-exact (optim.FusedAdam(lazy_tables=True)): rows a batch gathers / updates are replayed to "
                               "the current step in registers, bit-identical to the dense per-step update "
                               "(tests/test_lazy_tables_gpu.py); all other rows when the table is materialised"}
        if args.full or args.dump_outputs:
            behind = opt._step_count - opt._lazy_flushed_at
            torch.cuda.synchronize()
            tm0 = time.perf_counter()
            opt.materialize_tables()
            torch.cuda.synchronize()
            mat_ms = 1e3 * (time.perf_counter() - tm0)
            if args.full:
                tables_info.update({"full_materialize_ms": round(mat_ms, 3), "steps_replayed_per_row": behind,
                                    "amortized_ms_per_step": round(mat_ms / max(1, behind), 5),
                                    "note": "NOT inside the timed region: a checkpoint (model.state_dict()) pays "
                                            "full_materialize_ms once; ms_per_step + amortized_ms_per_step is the all-inclusive "
                                            "figure"})

    dumped = None
    if args.dump_outputs and rank == 0:
        dumped = dump_outputs(args.dump_outputs, final_loss_t, trainer, model)
        log(f"outputs of the last timed step: {dumped['arrays']} arrays, {dumped['bytes']} bytes under {dumped['dir']}")

    # per-kernel roofline: eager pass with HIP events around the hot C-ABI calls (rank 0's GPU; N = 1 only, so that the
    # collectives of the other ranks are not left waiting)
    roof_rows = []
    foreign_kernels = None
    if args.full and args.profile_steps > 0 and world == 1 and args.encoder == "densenet121" and not args.unfused_backbone:
        log(f"kernel timing pass: {args.profile_steps} eager steps, HIP events per C-ABI call")
        eager = TrainStep(model, opt, reducer, graphs=False)
        if getattr(model, "embedding_grad", "dense") == "rowsparse":
            model.sparse_grads.clear()                   # the eager pass owns the sink from here on
        roof_rows = kernel_roofline(lambda i: eager(batches[i % len(batches)]), args.profile_steps, model)
        # which kernels did a step launch?  One eager issue of exactly the sequence the step graph records, under
        # torch.profiler's kernel activity records (mclstexp_amd/kernel_audit.py; tests/test_own_kernels_gpu.py asserts the
        # same): library kernels (hipBLASLt Cijk_*, at::native::*, MIOpen) would be listed here by name
        try:
            from mclstexp_amd import kernel_audit
            eager.run_sequence_eager(batches[0])
            ks = kernel_audit.step_kernels(lambda: eager.run_sequence_eager(batches[1 % len(batches)]))
            foreign_kernels = {"kernel_records": sum(ks.values()), "distinct": len(ks),
                               "foreign": {n[:100]: ks[n] for n in kernel_audit.foreign(ks)}}
        except Exception as e:                       # the audit must never cost the bench line
            foreign_kernels = {"error": repr(e)[:200]}

    if rank == 0:
        steps_per_s = args.steps / dt
        gb = args.batch * world
        roof = None
        if roof_rows:
            roof = dict(roof_rows[0])
            roof["note"] = ("launch unit with the largest time per step; HIP events on the launch stream, eager pass "
                            "after the timed region, side streams off (each launch alone on the GPU)")
        out = {
            "metric": "training spots/sec (= steps/sec x global batch) at batch %d/GPU, %dpx patches, %d genes"
                      % (args.batch, args.image, args.genes),
            "value": round(steps_per_s * gb, 2), "unit": "spots/s", "steps_per_sec": round(steps_per_s, 4),
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(1e3 * dt / args.steps, 3), "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": "bf16" if bb is not None else "f32", "data": "synthetic",
            "config": {"workload": f"{baseline_config_name(args)}: train step, batch {args.batch}/GPU, "
                                   f"{args.image}x{args.image} patches, {args.genes} genes, {args.encoder} image encoder",
                       "global_batch": gb, "parallelism": f"dp{world}", "backbone_dtype": args.backbone_dtype,
                       "spot_path_mfma": args.compute, "infonce": args.infonce,
                       "infonce_effective": model.infonce_effective(gb), "hip_graphs": not args.no_graphs,
                       "optimizer": "Adam(lr=1e-4, wd=1e-3) incl. 2x(65536,G) tables",
                       "position_tables": tables_info,
                       "dp_semantics": "spot-encoder attention and BatchNorm statistics are per shard (per GPU); "
                                       "InfoNCE is global over the all-gathered embeddings",
                       "dp_backward_segments": (len(trainer.seg_graphs) + 1 if (dist_on and trainer.seg_graphs) else None),
                       "fallbacks": densenet_fused.fallback_counts(),
                       "step_kernel_audit": foreign_kernels,
                       "parity_at_benched_shape": parity_artifact(args) if args.full else None,
                       "final_loss": round(final_loss, 4),
                       "final_loss_note": f"{args.n_batches} synthetic batches are cycled: the loss reflects "
                                          "memorisation of that set, it is not a convergence claim"},
            "roofline": roof,
            "roofline_kernels": roof_rows[1:14],
            "roofline_step": ({
                "strict_algorithmic_bytes_per_step_listed_units": round(sum(r["strict_bytes_per_step"] for r in roof_rows), 1),
                "hbm_frac_of_step": round(sum(r["strict_bytes_per_step"] for r in roof_rows) / (dt / args.steps)
                                          / 1e9 / HBM_PEAK_GBS, 4),
                "step_tflops": round(2.21e12 / (dt / args.steps) / 1e12, 1) if baseline_config_name(args) == "BASELINE configs[1]" else None,
                "mfma_frac_of_step": round(2.21e12 / (dt / args.steps) / 1e12 / MFMA_BF16_PEAK_TFS, 4)
                if baseline_config_name(args) == "BASELINE configs[1]" else None,
                "note": "sum over the listed launch units of their strict algorithmic bytes per step / the TIMED step (graph "
                        "replay, lanes overlapped) / 8 TB/s; 2.21 TFLOP per step (SURVEY section 8d)"} if roof_rows else None),
        }
        if dumped is not None:
            out["outputs_dump"] = dumped
        if args.full and world == 1 and not args.no_cpu_baseline:
            log("gpu done: %.2f ms/step; timing the CPU oracle baseline" % out["ms_per_step"])
            out["cpu_baseline"] = cpu_baseline(args, args.cpu_budget_s)
        sys.stdout.flush()
        os.write(_RESULT_FD, (json.dumps(out) + "\n").encode())
    mdist.shutdown()


if __name__ == "__main__":
    main()
