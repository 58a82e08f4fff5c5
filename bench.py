#!/usr/bin/env python3
"""Headline benchmark (BASELINE.json): output tokens/sec of `lmstudio.chat_model`-style greedy
generation on a random-init Llama-3-8B Q4_K_M GGUF, plus the p50 NATS request-reply RTT.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--concurrency B] [--tp T] [--ep]
                    [--model llama-3-8b|llama-3-70b|mixtral-8x7b|...] [--device cuda|cpu]

One step = one continuous-batching decode step over B in-flight requests per model replica
(hipGraph replay + per-step scheduling + the host<-device next-token copy: the real serving
loop, nothing skipped).

A plain run sets up, warms up, times the K steps and prints the result line. `--full` adds what the
headline figure does not need: GPU clock / power telemetry over the timed region, the NATS RTTs, the
service-path load burst (`--serve-load`) and, on N > 1 GPUs, the tensor-parallel leg (`--tp-leg`).
`--dump-outputs DIR` writes the tokens the timed steps produced (`DIR/tokens.npy`, float32 [B, K];
`DIR/tokens_last_step.npy`, [B]); the same arguments give the same prompts and weights on every run.

Multi-GPU: `--gpus N` runs N ranks, one per GPU. Launched by `torch.distributed.run` (the driver
does this, setting WORLD_SIZE) or, when WORLD_SIZE is unset, bench.py starts
`torch.distributed.run` itself as a child process BEFORE touching the GPU and exits with its
code. The N ranks form N/T model replicas of T-way tensor parallelism:
  * T = 1 (default, BASELINE config 2): N independent replicas -- the reference's NATS
    queue-group scale-out (`/root/reference/README.md:478-484`); scaling is weak.
  * T > 1 (`--tp`, BASELINE config 3: Llama-3-70B TP=8): rank 0 of each replica schedules,
    the others replay its steps; row-parallel all-reduces over RCCL/xGMI.
  * `--ep` (BASELINE config 5: Mixtral): experts are owned whole by ranks (expert parallel).
Rank 0 prints ONE JSON line; `value` is the whole-job aggregate (sum over replicas of tokens /
max-over-ranks time of the K timed steps, bracketed by a world barrier + device sync).
"""
from __future__ import annotations

import argparse
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

METRIC = "output tokens/sec + p50 NATS req-reply RTT, Llama-3-8B Q4_K chat_model"


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1, help="ranks (one per GPU) of the job")
    ap.add_argument("--steps", type=int, default=200, help="timed decode steps (sustained run by default)")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--concurrency", type=int, default=512, help="in-flight chat requests per model replica")
    ap.add_argument("--prompt-len", type=int, default=128)
    ap.add_argument("--sample-frac", type=float, default=0.0,
                    help="fraction of the requests decoded with temperature 0.7 / top-p 0.95 / top-k 40 (device sampler)")
    ap.add_argument("--model", default="llama-3-8b")
    ap.add_argument("--ftype", default=None, help="default: Q5_K_M for mixtral, else Q4_K_M")
    ap.add_argument("--tp", type=int, default=1, help="tensor-parallel degree (divides --gpus)")
    ap.add_argument("--ep", action="store_true", help="MoE: expert parallel over the TP group")
    ap.add_argument("--device", default="cuda", choices=("cuda", "cpu"), help="cpu: gloo rehearsal of the path")
    ap.add_argument("--model-dir", default=os.environ.get("NLS_BENCH_DIR", "/tmp/nls_bench"))
    ap.add_argument("--no-graphs", action="store_true")
    ap.add_argument("--no-rtt", action="store_true")
    ap.add_argument("--single-stream", action="store_true", help="also time batch-1 decode (reported, not the headline)")
    ap.add_argument("--serve-load", type=int, default=512,
                    help="after the timed region: N concurrent lmstudio.chat_model requests through NATS (half "
                         "sampled at temperature 0.7) against the same engine; 0 disables")
    ap.add_argument("--serve-tokens", type=int, default=256, help="max_tokens of each --serve-load request")
    ap.add_argument("--prefill-tokens", type=int, default=int(os.environ.get("NLS_BENCH_PREFILL_TOKENS", "4096")),
                    help="the engine's prefill chunk (tokens per prefill forward; the worker's default; EP: <= 2048)")
    ap.add_argument("--tp-leg", type=int, default=1,
                    help="with --gpus N > 1 and --tp 1: also measure Llama-3-70B over all N ranks (tensor parallel; "
                         "reported as tp_leg); 0 disables")
    ap.add_argument("--tp-leg-model", default=None,
                    help="model of the TP leg (default llama-3-70b; on --device cpu llama-3-70b-1layer)")
    ap.add_argument("--tp-leg-concurrency", type=int, default=64)
    ap.add_argument("--tp-leg-timeout", type=float, default=480.0,
                    help="seconds before the TP leg is abandoned (bounds what it adds to an N-GPU run)")
    ap.add_argument("--step-breakdown", action="store_true",
                    help="report host time vs time blocked on the previous step's tokens (diagnostic)")
    ap.add_argument("--full", action="store_true",
                    help="also measure what the headline figure does not need: GPU clock / power telemetry over the "
                         "timed region, the NATS RTTs, the --serve-load burst and, on N > 1 GPUs, the TP leg")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write the tokens they produced as DIR/<name>.npy (float32)")
    a = ap.parse_args(argv)
    if a.ftype is None:
        a.ftype = "Q5_K_M" if "mixtral" in a.model else "Q4_K_M"
    return a


def _free_port() -> int:
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def spawn(args, argv) -> int:
    """--gpus N > 1 without a launcher: run torch.distributed.run as a CHILD process (this process
    has not imported torch, let alone touched the GPU) and return its exit code."""
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr=127.0.0.1", f"--master-port={_free_port()}", os.path.abspath(__file__), *argv]
    return subprocess.call(cmd, env=env)


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    args = parse(argv)
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        return spawn(args, argv)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        raise SystemExit(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}: launch one rank per GPU")
    if world % args.tp:
        raise SystemExit(f"bench.py: --tp {args.tp} must divide --gpus {world}")
    return run(args, world)


def _setup(args, world: int):
    import torch
    import torch.distributed as dist
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    cuda = args.device == "cuda"
    if cuda:
        torch.cuda.set_device(local)
        dev = torch.device("cuda", local)
    else:
        dev = torch.device("cpu")
        torch.set_num_threads(max(1, min(4, (os.cpu_count() or 2) // max(1, world))))
    if world > 1:
        import datetime
        kw = dict(backend="nccl" if cuda else "gloo", timeout=datetime.timedelta(seconds=1800))
        if cuda:
            kw["device_id"] = dev
        dist.init_process_group(**kw)
    return rank, local, cuda, dev


def _tp_comm(world: int, tp: int, rank: int, cuda: bool, dev):
    """This rank's tensor-parallel communicator (RCCL data plane + gloo/shm control, one-shot IPC AR)."""
    import torch.distributed as dist
    from nats_llm_studio_amd.parallel.comm import Comm
    mine = None
    for g in range(world // tp):     # every rank creates every group, in the same order
        ranks = list(range(g * tp, (g + 1) * tp))
        pg = dist.new_group(ranks) if world > tp else dist.group.WORLD
        cg = dist.new_group(ranks, backend="gloo") if cuda else pg
        if g == rank // tp:
            mine = (pg, cg)
    comm = Comm(mine[0], mine[1], dev)
    if cuda and os.environ.get("NLS_ONESHOT_AR", "1") == "1":
        from nats_llm_studio_amd.parallel.oneshot import try_oneshot
        comm.oneshot = try_oneshot(comm)
    return comm


def run(args, world: int):
    import torch
    import torch.distributed as dist
    rank, local, cuda, dev = _setup(args, world)
    leg = _leg(args, world, rank, local, cuda, dev, args.model, args.ftype, args.tp, args.ep, args.concurrency,
               args.steps, args.warmup, headline=True)
    if args.full and world > 1 and args.tp == 1 and args.tp_leg > 0:
        # --full dp runs on N > 1 GPUs also measure the tensor-parallel data plane: the 70B model over all N GPUs
        # (BASELINE config 3), reported next to the headline as "tp_leg". It runs as a CHILD job (its own
        # torch.distributed.run, started by rank 0 once every rank has freed its headline model) under a
        # time limit, so a TP problem costs the leg, never the headline measurement.
        leg["info"].pop("model", None)
        leg.pop("eng", None)
        import gc
        gc.collect()
        if cuda:
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
        ctrl = dist.new_group(backend="gloo") if cuda else None
        dist.barrier(group=ctrl)
        if rank == 0:
            leg["extra"]["tp_leg"] = _run_tp_leg(args, world, cuda)
        dist.barrier(group=ctrl)
    _reduce_and_report(args, world, dist, torch, dev, leg["elapsed"], leg["tokens"], leg["info"], rank)
    if world > 1:
        dist.destroy_process_group()
    return 0


def _run_tp_leg(args, world: int, cuda: bool) -> dict:
    tmodel = args.tp_leg_model or ("llama-3-70b" if cuda else "llama-3-70b-1layer")
    if cuda and _skip_tp_leg(args, tmodel):
        import shutil
        free = shutil.disk_usage(args.model_dir).free
        return {"skipped": f"{free / 1e9:.0f} GB free in {args.model_dir}; the {tmodel} GGUF needs ~43 GB"}
    cmd = [sys.executable, os.path.abspath(__file__), "--gpus", str(world), "--tp", str(world), "--model", tmodel,
           "--ftype", "Q4_K_M", "--steps", str(args.steps), "--warmup", str(args.warmup), "--concurrency",
           str(args.tp_leg_concurrency), "--prompt-len", str(args.prompt_len), "--no-rtt", "--serve-load", "0",
           "--tp-leg", "0", "--device", args.device, "--model-dir", args.model_dir]
    env = {k: v for k, v in os.environ.items()
           if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "LOCAL_WORLD_SIZE", "GROUP_RANK", "ROLE_RANK",
                        "ROLE_WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT", "TORCHELASTIC_RUN_ID",
                        "TORCHELASTIC_RESTART_COUNT", "TORCHELASTIC_MAX_RESTARTS", "GROUP_WORLD_SIZE",
                        "ROLE_NAME", "TORCH_NCCL_ASYNC_ERROR_HANDLING")}
    t0 = time.time()
    # its own session: at the time limit the WHOLE process group goes (the launcher and every rank it started),
    # so no rank of an abandoned leg keeps a GPU for the runs after this one
    p = subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env,
                         start_new_session=True)
    try:
        out, err = p.communicate(timeout=args.tp_leg_timeout)
    except subprocess.TimeoutExpired:
        import signal
        try:
            os.killpg(p.pid, signal.SIGKILL)
        except ProcessLookupError:
            pass
        p.communicate()
        return {"model": f"{tmodel} Q4_K_M", "parallelism": f"tp{world}",
                "error": f"no result within {args.tp_leg_timeout} s (process group killed)"}
    lines = [l for l in out.splitlines() if l.startswith("{")]
    if p.returncode != 0 or not lines:
        return {"model": f"{tmodel} Q4_K_M", "parallelism": f"tp{world}", "error": f"rc {p.returncode}",
                "stderr_tail": err[-600:]}
    d = json.loads(lines[-1])
    return {"model": d["config"]["model"], "parallelism": d["config"]["parallelism"],
            "concurrency": args.tp_leg_concurrency, "value": d["value"], "unit": d["unit"],
            "ms_per_step": d["ms_per_step"], "steps": d["steps"], "weights_gb_per_rank": d["weights_gb_per_rank"],
            "comm": d["comm"], "timings_s": d["timings_s"], "wall_s": round(time.time() - t0, 1)}


def _skip_tp_leg(args, tmodel: str) -> bool:
    """The 70B GGUF needs ~43 GB of disk next to the 8B one: skip (and say so) where there is no room."""
    import shutil
    os.makedirs(args.model_dir, exist_ok=True)
    have = os.path.exists(os.path.join(args.model_dir, f"{tmodel}-Q4_K_M.gguf"))
    return not have and shutil.disk_usage(args.model_dir).free < 50e9


def _leg(args, world, rank, local, cuda, dev, model_name, ftype, tp, ep, B, steps, warmup, headline):
    """One measured configuration: N/tp replicas of `model_name`, B in-flight requests per replica,
    `warmup` untimed then `steps` timed decode steps bracketed by a world barrier + device sync."""
    import numpy as np
    import torch
    import torch.distributed as dist
    sync = torch.cuda.synchronize if cuda else (lambda *a: None)
    tp_rank = rank % tp
    comm = _tp_comm(world, tp, rank, cuda, dev) if tp > 1 else None

    from nats_llm_studio_amd import build as nbuild
    from nats_llm_studio_amd.gguf.reader import GGUFReader
    from nats_llm_studio_amd.gguf.synth import write_synthetic_gguf
    from nats_llm_studio_amd.models.llama import LlamaModel, ShardSpec
    from nats_llm_studio_amd.engine.engine import Engine, GenRequest
    from nats_llm_studio_amd.engine.sampling import SamplingParams

    path = os.path.join(args.model_dir, f"{model_name}-{ftype}.gguf")
    t0 = time.time()
    if local == 0:
        if cuda:
            nbuild.build_kernels()
        if not os.path.exists(path):
            os.makedirs(args.model_dir, exist_ok=True)
            write_synthetic_gguf(path, model_name, ftype, seed=0)
    if world > 1:
        dist.barrier()
    t_gen = time.time() - t0

    t0 = time.time()
    reader = GGUFReader(path)
    model = LlamaModel(reader, dev, ShardSpec(tp_rank, tp, ep), comm)
    sync()
    t_load = time.time() - t0

    max_prefill = min(args.prefill_tokens, 2048) if ep else args.prefill_tokens
    # sequences prefilled early already decode while later ones prefill: budget those steps too
    prefill_steps = (B * args.prompt_len + max_prefill - 1) // max_prefill
    gen_tokens = warmup + steps + prefill_steps + 8
    need_tokens = args.prompt_len + gen_tokens
    serve = headline and args.serve_load > 0
    # the headline engine later serves the --serve-load burst (prompts up to 1.5x --prompt-len + serve_tokens):
    # its context covers those, and on GPUs the KV pool takes the engine's default share of free HBM
    # (blocks are allocated as sequences grow, so pool size costs nothing in the timed decode steps)
    serve_ctx = (3 * args.prompt_len // 2 + 16 + args.serve_tokens + 16) if serve else 0
    ctx = max(need_tokens + 16, 512, serve_ctx)
    eng = Engine(model, None, max_batch=B, max_prefill_tokens=max_prefill, use_graphs=cuda and not args.no_graphs,
                 ctx=ctx, num_blocks=None if cuda else B * ((need_tokens + 15) // 16 + 1))
    marks = []
    info_mem = dict(dense_gb=round(eng.dense_bytes / 1e9, 2), kv_pool_gb=round(eng.kv_pool_bytes / 1e9, 2))
    if dev.type == "cuda":
        # HBM still free after weights, copies and KV pool: what a larger pool / more requests could use
        info_mem["hbm_free_gb"] = round(torch.cuda.mem_get_info(dev)[0] / 1e9, 1)

    def barrier_hook():                 # both sides of the timed region, on every rank
        sync()
        if world > 1:
            dist.barrier()
        sync()
        marks.append(time.perf_counter())

    info = dict(B=B, tp=tp, weights_gb=round(model.weight_bytes / 1e9, 3), n_expert=model.cfg.n_expert,
                timings={"gguf_write": round(t_gen, 1), "load": round(t_load, 1)}, **info_mem)
    out = dict(elapsed=0.0, tokens=0.0, info=info, extra={})
    leader = tp_rank == 0
    if not leader:                      # follower: replay the leader's steps until STOP
        eng.sync_hook = barrier_hook
        eng.follow()
        out["elapsed"] = marks[1] - marks[0] if len(marks) >= 2 else 0.0
        info.update(model=model, comm_stats=None, rtt=None, chat_rtt=None, t_prefill=0.0, extra=out["extra"])
        return out

    eng.capture_all()
    rng = np.random.default_rng(rank)
    vocab = model.cfg.vocab
    nsamp = int(round(args.sample_frac * B))        # rows decoded with the reference payload's sampling

    def params(i):
        if i < nsamp:
            return SamplingParams(max_tokens=gen_tokens, ignore_eos=True, temperature=0.7, top_p=0.95, top_k=40,
                                  seed=i)
        return SamplingParams(max_tokens=gen_tokens, ignore_eos=True)
    futs = [eng.submit(GenRequest(list(rng.integers(0, min(vocab, 100000), args.prompt_len)), params(i)))
            for i in range(B)]
    # prefill every request (not timed), then warm up the decode loop
    t0 = time.time()
    while any(s.n_prefilled < s.n_target for s in eng.running) or eng.waiting:
        eng.step()
    sync()
    t_prefill = time.time() - t0
    info["timings"]["prefill_all"] = round(t_prefill, 3)
    for _ in range(warmup):
        eng.step()
    assert len(eng.running) == B, "all requests must still be decoding in the timed region"

    wait = [0.0]
    orig = eng._process
    if args.step_breakdown and cuda and headline:    # time the host spends blocked on step N's event
        def timed_outer(infl):
            t = time.perf_counter()
            eng._ev[infl[1]].synchronize()
            wait[0] += time.perf_counter() - t
            orig(infl)
        eng._process = timed_outer
    extra = out["extra"]
    st0 = dict(comm.stats) if comm is not None else None
    telem = None
    if cuda and headline and args.full:      # GFX clock / power / temperature at both brackets and in between
        from nats_llm_studio_amd.utils.telemetry import GpuTelemetry
        telem = GpuTelemetry(local)
    eng.sync(barrier_hook) if tp > 1 else barrier_hook()
    if telem is not None:
        telem.start()
    for _ in range(steps):
        eng.step()
    eng.sync(barrier_hook) if tp > 1 else barrier_hook()
    if telem is not None:
        telem.stop()
        extra["gpu_telemetry"] = telem.summary()
    elapsed = marks[1] - marks[0]
    eng._process = orig
    if args.dump_outputs:
        _dump_outputs(args.dump_outputs, eng, futs, steps, rank)
    comm_stats = None
    if comm is not None:
        d = {k: comm.stats[k] - st0.get(k, 0) for k in comm.stats}
        comm_stats = {"all_reduce_per_step": round(d["all_reduce"] / steps, 2),
                      "all_reduce_bytes_per_step": int(d["all_reduce_bytes"] / steps),
                      "ctrl_msgs_per_step": round(d["ctrl"] / steps, 2),
                      "ctrl_us_per_step": round(d["ctrl_s"] / steps * 1e6, 1),
                      "ctrl_transport": "shm-ring" if comm.ring is not None else "gloo",
                      "oneshot": comm.oneshot is not None}

    if args.step_breakdown and cuda and headline:
        eng._drain()
        g = eng.graphs.get((eng._bucket(B), False))
        replay = None
        if g is not None and tp == 1:   # GPU-only replay of the same decode graph (diagnostic)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            g.replay()
            e0.record()
            for _ in range(10):
                g.replay()
            e1.record()
            sync()
            replay = round(e0.elapsed_time(e1) / 10, 3)
        extra["step_breakdown_ms"] = {"gpu_wait": round(wait[0] / steps * 1e3, 3),
                                      "host_other": round((elapsed - wait[0]) / steps * 1e3, 3),
                                      "graph_replay_only": replay}
    moe = getattr(eng.db, "moe", None)
    if cuda and moe and "counts" in moe:   # routed rows per local expert, last MoE layer of the last step
        sync()
        extra["moe_counts_last_layer"] = moe["counts"][:len(model.experts)].tolist()
    if args.full or args.single_stream:     # drain: the legs below run on the idle engine
        while eng.running or eng.waiting:
            eng.step()
        for f in futs:
            f.result()
    if args.single_stream and headline:
        r = eng.generate(list(rng.integers(0, 1000, args.prompt_len)), SamplingParams(max_tokens=64, ignore_eos=True))
        extra["single_stream_tok_s"] = round(r.tokens_per_second, 1)
        extra["single_stream_ttft_ms"] = round(r.time_to_first_token * 1e3, 2)

    rtt = chat_rtt = None
    if args.full and headline and not args.no_rtt and rank == 0:
        try:
            from nats_llm_studio_amd.service.bench_rtt import measure_rtt
            rtt = measure_rtt(n=500)
        except Exception as e:  # natscore missing -> report null, never fake
            extra["rtt_error"] = str(e)[:200]
        try:   # chat_model on the real engine (after the timed region; engine idle)
            from nats_llm_studio_amd.service.bench_rtt import measure_engine_chat_rtt
            chat_rtt = measure_engine_chat_rtt(eng, reader.metadata, n=30)
        except Exception as e:
            extra["chat_rtt_error"] = str(e)[:300]
        if serve and tp == 1:
            try:   # service-path throughput: concurrent chat_model burst through natscore
                from nats_llm_studio_amd.service.bench_rtt import measure_engine_chat_load
                extra["service_load"] = measure_engine_chat_load(eng, reader.metadata, n=args.serve_load,
                                                                 max_tokens=args.serve_tokens,
                                                                 prompt_tokens=args.prompt_len)
            except Exception as e:
                extra["service_load_error"] = str(e)[:300]
    eng.stop_followers()
    info.update(model=model, rtt=rtt, chat_rtt=chat_rtt, comm_stats=comm_stats, t_prefill=t_prefill, extra=extra)
    out.update(elapsed=elapsed, tokens=float(B * steps), eng=eng)
    return out


def _dump_outputs(d, eng, futs, steps, rank):
    """What the timed steps returned to their callers: each request's token of every timed step, in
    submission order (`tokens.npy`, [B, steps]), and of the last one alone (`tokens_last_step.npy`, [B]).
    Token ids are exact in float32 (vocab < 2**24). Replica leaders other than rank 0 add `.rank<r>`."""
    import numpy as np
    eng._drain()                        # the last timed step's tokens are still in flight on the host side
    seq = {id(s.fut): s for s in eng.running}
    toks = np.asarray([seq[id(f)].generated[-steps:] for f in futs], dtype=np.float32)
    assert toks.shape == (len(futs), steps), toks.shape
    os.makedirs(d, exist_ok=True)
    sfx = "" if rank == 0 else f".rank{rank}"
    np.save(os.path.join(d, f"tokens{sfx}.npy"), toks)
    np.save(os.path.join(d, f"tokens_last_step{sfx}.npy"), np.ascontiguousarray(toks[:, -1]))


def _reduce_and_report(args, world, dist, torch, dev, elapsed, tokens, info, rank):
    t_max, tok_sum = elapsed, tokens
    if world > 1:
        tt = torch.tensor([elapsed, tokens], dtype=torch.float64, device=dev)
        mx = tt.clone()
        dist.all_reduce(mx, op=dist.ReduceOp.MAX)
        dist.all_reduce(tt, op=dist.ReduceOp.SUM)
        t_max, tok_sum = float(mx[0]), float(tt[1])
    if rank != 0:
        return
    B, tp = info["B"], info["tp"]
    dp = world // tp
    par = f"dp{dp}" if tp == 1 else (f"tp{tp}" if dp == 1 else f"dp{dp}xtp{tp}")
    if args.ep and info["n_expert"]:
        par += "+ep"
    rtt, chat_rtt = info["rtt"], info["chat_rtt"]
    out = {
        "metric": METRIC,
        "value": round(tok_sum / t_max, 2),
        "unit": "output tokens/s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": round(t_max / args.steps * 1e3, 4),
        "higher_is_better": True,
        "scaling": "weak" if tp == 1 else "strong",   # tp: one replica's fixed batch over more GPUs
        "vs_baseline": None,
        "dtype": "fp16",   # f16 activations + f16 MFMA on K-quant weights, fp32 accumulate and residual
        "data": f"synthetic prompts, random-init GGUF weights ({args.ftype} mix), no network",
        "config": {
            "model": f"{args.model} {args.ftype}",
            "global_batch": B * dp,
            "seq_len": args.prompt_len,
            "parallelism": par,
            "concurrency_per_replica": B,
            "hipgraph": args.device == "cuda" and not args.no_graphs,
            "device": args.device,
            "sampled_frac": args.sample_frac,
        },
        "p50_rtt_ms": (chat_rtt or {}).get("p50_ms", None if rtt is None else rtt.get("p50_ms")),
        "rtt_chat_model_engine": chat_rtt,
        "rtt": rtt,
        "weights_gb_per_rank": info["weights_gb"],
        "dense_weight_copies_gb": info.get("dense_gb"),
        "kv_pool_gb": info.get("kv_pool_gb"),
        "hbm_free_gb": info.get("hbm_free_gb"),
        "comm": info["comm_stats"],
        "timings_s": info["timings"],
        "kernels_stamp_current": _kernels_current(),
        **info["extra"],
    }
    print(json.dumps(out), flush=True)


def _kernels_current():
    """Whether _kernels.so carries the content stamp of this tree's kernel sources (build.py)."""
    try:
        from nats_llm_studio_amd import build
        return build.kernels_current()
    except Exception:
        return None


if __name__ == "__main__":
    rc = main()
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        # multi-rank: results are printed and the process groups destroyed; skip interpreter teardown,
        # where torch's gloo helper threads occasionally abort on a still-joinable std::thread
        # ("terminate called without an active exception", ~1 in 6 CPU tp2+ep runs)
        sys.stdout.flush()
        sys.stderr.flush()
        os._exit(rc or 0)
    sys.exit(rc)
