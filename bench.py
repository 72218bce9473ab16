#!/usr/bin/env python3
"""Flagship serving benchmark — MCP tool_call -> gRPC unary req/sec.

Measures the BASELINE.json headline metric on the MI355X-native gateway.
The default config (hello1k) is the REAL SERVING path end to end: the C++
closed-loop load generator opens `--batch` keep-alive HTTP sessions against
the native gateway (C++ epoll reactors -> C++ session guard -> GIL-free
span executor: GPU envelope parse + JSON->protobuf k_json2pb, real gRPC
unary invokes against a local backend process over the native h2
transport, GPU protobuf->JSON + response envelopes k_pb2json).  One
"step" = every session completing one request; p50_rtt_ms is the measured
per-request round-trip median from the closed-loop client (NOT a batch
step time — VERDICT r1 item 8).  The reference (aalobaidi/ggRMCP)
publishes no numbers, so vs_baseline is null.

Contract (driver):
  python bench.py --gpus N --steps K --warmup W
launched for N>1 as one rank per GPU via torch.distributed.run; rank 0
prints ONE JSON line; value = WHOLE-JOB req/s over all ranks (weak scaling:
each rank runs its own gateway + sessions + backend shard; discovery state
is broadcast over RCCL/gloo first).  Such a plain run sets up, warms up,
times the K steps and prints the line, nothing else.  --dump-outputs DIR
also writes one step's response bodies as .npy arrays (same arguments ->
same inputs -> comparable outputs across builds); --full is where any
secondary measurement belongs (none exist today: every other workload is a
--config run of its own).

Configs (BASELINE.json):
  --config hello1k   SERVING: hello SayHello, 1 KB bodies, --batch sessions
                     of real HTTP through the native gateway (default)
  --config pipeline  the batch pipeline alone (no HTTP ingest; round-1 mode)
  --config wide64    synthetic 64-field proto, 64 KB payloads, validation on
  --config stream    server-streaming StreamEcho, N msgs/stream (config 4)
  --config multi     4 backends, mixed unary+stream, headers on (config 5)
  --config cpu       reference-equivalent CPU-only plumbing path (config 1)
"""

from __future__ import annotations

import argparse
import json
import os
import random
import statistics
import subprocess
import sys
import tempfile
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent))

from ggrmcp_amd.backend.discovery import ServiceDiscoverer  # noqa: E402
from ggrmcp_amd.config import Config  # noqa: E402
from ggrmcp_amd.utils.synthetic import (  # noqa: E402
    hello_payload,
    jsonrpc_body,
    wide_payload,
)


def parse_args():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    # defaults size the timed region to SECONDS (serving: steps x batch
    # requests), so the driver's GPU-busy sampler sees the run (VERDICT r1
    # item 8: 20 x 4 ms was a 0.08 s window)
    ap.add_argument("--steps", type=int, default=-1,
                    help="-1 = config default (serving 800, pipeline 200)")
    ap.add_argument("--warmup", type=int, default=-1,
                    help="-1 = config default (serving 40, pipeline 20)")
    ap.add_argument("--config", default="hello1k",
                    choices=["hello1k", "pipeline", "wide64", "stream",
                             "multi", "cpu"])
    ap.add_argument("--client-threads", type=int, default=16,
                    help="load-generator threads (serving config); 16 "
                         "beats 8 by ~11%% at 1024 sessions")
    ap.add_argument("--stream-depth", type=int, default=4096,
                    help="messages per stream (config 4)")
    ap.add_argument("--backends", type=int, default=4,
                    help="backend count for the multi config (config 5)")
    ap.add_argument("--batch", type=int, default=1024, help="requests per step (= concurrent sessions)")
    ap.add_argument("--payload-bytes", type=int, default=0)
    ap.add_argument("--invoke-workers", type=int, default=64)
    ap.add_argument("--backend-workers", type=int, default=32)
    ap.add_argument("--transport", default="native", choices=["native", "grpcio"],
                    help="wire invoker: native C++ h2 client or grpcio threads")
    ap.add_argument("--backend", default="native", choices=["native", "python"],
                    help="local bench backend implementation")
    ap.add_argument("--connections", type=int, default=0,
                    help="native transport connections per backend "
                         "(0 = auto: 8, or 16 for wide64 whose 128 MB/step "
                         "is UDS-syscall bound — profiles/wide64_conns.log)")
    ap.add_argument("--streams", type=int, default=0,
                    help="override config.gpu.streams (engine instances)")
    ap.add_argument("--reactors", type=int, default=0,
                    help="override config.server.reactors (serving config)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write the response bodies of "
                         "one step as DIR/<name>.npy (float32/float64, "
                         "<= 64 MB; see dump_outputs)")
    ap.add_argument("--full", action="store_true",
                    help="also run the secondary measurements and checks.  "
                         "A plain run does only what the headline figure "
                         "needs; this benchmark has no secondary work of its "
                         "own (other workloads are separate --config runs), "
                         "so today --full runs exactly the plain run")
    return ap.parse_args()


def start_backend(rank: int, workers: int, native: bool, package: str = "bench",
                  index: int = 0):
    """Backend in its own process over a unix socket (no shared GIL)."""
    sock = os.path.join(
        tempfile.gettempdir(), f"ggrmcp_bench_{os.getpid()}_{rank}_{index}.sock"
    )
    if os.path.exists(sock):
        os.unlink(sock)
    cmd = [sys.executable, "-m", "examples.bench_backend", "--uds", sock,
           "--workers", str(workers), "--package", package]
    if native:
        cmd.append("--native")
    proc = subprocess.Popen(
        cmd,
        stdout=subprocess.PIPE, stderr=subprocess.DEVNULL,
        cwd=str(Path(__file__).resolve().parent), text=True,
    )
    line = proc.stdout.readline()
    if not line.startswith("READY"):
        raise RuntimeError(f"backend failed to start: {line!r}")
    return proc, sock


def make_bodies(cfg_name: str, batch: int, payload_bytes: int, seed: int,
                stream_depth: int = 4096, n_backends: int = 4):
    rng = random.Random(seed)
    bodies = []
    if cfg_name in ("hello1k", "pipeline", "cpu"):
        tool = "hello_helloservice_sayhello"
        size = payload_bytes or 1024
        for i in range(batch):
            bodies.append(jsonrpc_body(tool, hello_payload(rng, size), i + 1))
    elif cfg_name == "stream":
        # BASELINE config 4: server-streaming, N msgs/stream
        size = payload_bytes or 1024
        for i in range(batch):
            args = wide_payload(rng, target_bytes=size)
            args["f02Int32"] = stream_depth
            bodies.append(jsonrpc_body("bench_echoservice_streamecho", args, i + 1))
    elif cfg_name == "multi":
        # BASELINE config 5: mixed unary+stream across N backends, headers on
        size = payload_bytes or 4096
        for i in range(batch):
            be = i % n_backends
            args = wide_payload(rng, target_bytes=size)
            if i % 8 == 7:  # 1-in-8 requests is a stream
                args["f02Int32"] = 16
                tool = f"bench{be}_echoservice_streamecho"
            else:
                tool = f"bench{be}_echoservice_echo"
            bodies.append(jsonrpc_body(tool, args, i + 1))
    else:
        tool = "bench_echoservice_echo"
        size = payload_bytes or 64 * 1024
        for i in range(batch):
            bodies.append(jsonrpc_body(tool, wide_payload(rng, target_bytes=size), i + 1))
    return bodies


def http_step_responses(host: str, port: int, body: bytes, sessions: int,
                        timeout_s: float = 30.0):
    """One serving step seen from the client side: `sessions` keep-alive
    connections each POST `body` once (all in flight together, the way the
    load generator's sessions are) and the response BODIES come back in
    session order."""
    import socket

    socks = []
    try:
        for s in range(sessions):
            sk = socket.create_connection((host, port), timeout=timeout_s)
            sk.setsockopt(socket.IPPROTO_TCP, socket.TCP_NODELAY, 1)
            socks.append(sk)
        for s, sk in enumerate(socks):
            sk.sendall(
                b"POST / HTTP/1.1\r\nHost: b\r\n"
                b"Content-Type: application/json\r\n"
                b"Mcp-Session-Id: dump-%d\r\nContent-Length: %d\r\n\r\n"
                % (s, len(body)) + body)
        out = []
        for sk in socks:
            buf = b""
            while True:
                he = buf.find(b"\r\n\r\n")
                if he >= 0:
                    head = buf[:he].lower()
                    p = head.find(b"content-length:")
                    if p < 0:
                        raise RuntimeError(f"no Content-Length: {buf[:200]!r}")
                    cl = int(head[p + 15:].split(b"\r\n", 1)[0])
                    if len(buf) >= he + 4 + cl:
                        out.append(buf[he + 4:he + 4 + cl])
                        break
                chunk = sk.recv(1 << 16)
                if not chunk:
                    raise RuntimeError("gateway closed a dump connection")
                buf += chunk
        return out
    finally:
        for sk in socks:
            sk.close()


# float32 elements written to responses.npy at most (48 MB, so the whole
# dump stays under 64 MB with the two small index arrays)
DUMP_MAX_ELEMS = 12 * 1024 * 1024


def dump_outputs(out_dir: str, responses) -> None:
    """Write one step's response bodies (what a caller of the timed path
    receives) as .npy arrays:

      responses.npy         float32 [rows, width]: the bytes of each sampled
                            response, padded with -1 to the longest one
      response_rows.npy     float64 [rows]: which responses were sampled
                            (all of them when they fit; otherwise a fixed,
                            seeded sample in ascending order)
      response_lengths.npy  float64 [n]: byte length of EVERY response

    A step whose responses exceed the size budget keeps whole rows; only
    when a single response is larger than the budget is it cut to a prefix.
    """
    import numpy as np

    n = len(responses)
    lengths = np.array([len(r) for r in responses], dtype=np.float64)
    width = min(int(lengths.max()) if n else 0, DUMP_MAX_ELEMS)
    rows = min(n, max(1, DUMP_MAX_ELEMS // max(1, width)))
    picked = (list(range(n)) if rows >= n
              else sorted(random.Random(20240607).sample(range(n), rows)))
    arr = np.full((len(picked), width), -1.0, dtype=np.float32)
    for k, i in enumerate(picked):
        r = np.frombuffer(bytes(responses[i])[:width], dtype=np.uint8)
        arr[k, :r.size] = r
    os.makedirs(out_dir, exist_ok=True)
    np.save(os.path.join(out_dir, "responses.npy"), arr)
    np.save(os.path.join(out_dir, "response_rows.npy"),
            np.array(picked, dtype=np.float64))
    np.save(os.path.join(out_dir, "response_lengths.npy"), lengths)


def main() -> None:
    args = parse_args()
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", str(rank)))

    import torch

    use_gpu = args.config != "cpu" and torch.cuda.is_available()
    # per-config step defaults sized so the timed region spans seconds on
    # the GPU box yet finishes within minutes anywhere
    step_defaults = {
        "hello1k": (800, 40) if use_gpu else (5, 1),
        "pipeline": (200, 20),
        "wide64": (100, 10),
        "stream": (8, 2),
        "multi": (200, 20),
        "cpu": (5, 1),
    }
    if args.steps < 0:
        args.steps = step_defaults[args.config][0]
    if args.warmup < 0:
        args.warmup = step_defaults[args.config][1]
    # device index: clamp by the visible device count so a world-2 rehearsal
    # on a 1-GPU box maps both ranks onto cuda:0 (no-op on a full node)
    dev = (local_rank % max(1, torch.cuda.device_count())) if use_gpu else 0
    dist = None
    dist_backend = None
    if world > 1:
        import torch.distributed as dist_mod

        dist = dist_mod
        # GGRMCP_DIST_BACKEND=gloo lets the multi-rank GPU path be smoked on
        # a single GPU (RCCL refuses two ranks on one device)
        dist_backend = os.environ.get("GGRMCP_DIST_BACKEND") or (
            "nccl" if use_gpu else "gloo"
        )
        if use_gpu:
            torch.cuda.set_device(dev)
        dist.init_process_group(backend=dist_backend)

    # config 5 runs N distinct-package backends; both stream and multi can
    # use the native backend (h2grpc stream_echo route) with the batched
    # native streaming client
    native_backend = args.backend == "native"
    n_backends = args.backends if args.config == "multi" else 1
    backend_procs, socks = [], []
    for b in range(n_backends):
        pkg = f"bench{b}" if args.config == "multi" else "bench"
        proc, sock = start_backend(rank, args.backend_workers, native_backend,
                                   package=pkg, index=b)
        backend_procs.append(proc)
        socks.append(sock)
    backend_proc, sock = backend_procs[0], socks[0]
    gw = None
    try:
        cfg = Config.default()
        cfg.grpc.uds = sock
        cfg.gpu.enabled = use_gpu
        if args.config == "hello1k" and use_gpu:
            # tuned serving defaults (profiles/serving_sweep_r02.log):
            # reactors 4->8 and span engines 2->6 lifted 1-GPU serving
            # 242k -> 363k req/s; reactors 8->12 (after the flush-path
            # epoll_ctl fix) a further 379k -> 426k at 800 steps on a
            # 256-core box (gpurun_out/cf_r12t16.json).  Explicit flags
            # still override.  Multi-rank weak scaling shares the node's
            # cores across ranks, so shed reactors and client threads
            # there (the load generator competes hardest).
            cfg.gpu.streams = 6
            cfg.server.reactors = 12 if world == 1 else 6
            if world > 1 and args.client_threads == 16:
                args.client_threads = 8
        if args.streams > 0:
            cfg.gpu.streams = args.streams
        if args.reactors > 0:
            cfg.server.reactors = args.reactors
        if args.config == "wide64":
            # 64 KB payloads need bigger arenas.  Keep the batch LARGE: the
            # transcode kernels are per-wave latency-bound, so wall time per
            # dispatch is nearly flat in wave count — more requests in
            # flight is almost free GPU-side (profiles/wide64_kernels.txt)
            cfg.gpu.pinned_pool_bytes = 2 * 1024 * 1024 * 1024
            cfg.gpu.device_pool_bytes = 6 * 1024 * 1024 * 1024
            if args.streams <= 0:
                # 128 MB/step of staging wants more copy overlap than the
                # small-payload default (profiles/wide64_streams.log:
                # 4 engines 30-34k vs 2 engines 27-29k req/s)
                cfg.gpu.streams = 4
        if args.config == "stream" and args.batch == 1024:
            args.batch = 64  # 64 streams x 4096 msgs per step
        if args.config == "multi" and args.batch == 1024:
            args.batch = 512
        backend_cfgs = None
        if n_backends > 1:
            import dataclasses as _dc

            backend_cfgs = [
                _dc.replace(cfg.grpc, uds=s) for s in socks
            ]
        discoverer = ServiceDiscoverer(cfg, backends=backend_cfgs)
        shard_group = None
        if dist is not None:
            from ggrmcp_amd.parallel.dist import ShardGroup

            shard_group = ShardGroup.attach(
                dist, device=dev if (use_gpu and dist_backend == "nccl") else None
            )
        if native_backend or n_backends > 1:
            # no-reflection path: rank 0 builds the descriptor blob per
            # backend (the descriptor-set path, loader.go route) and
            # broadcasts it to the other shards over RCCL (parallel/dist.py)
            if rank == 0 or shard_group is None:
                from examples.protos import ALL_FDPS
                from ggrmcp_amd.utils.synthetic import synthetic_fdp
                from google.protobuf import descriptor_pb2

                for b in range(n_backends):
                    pkg = f"bench{b}" if n_backends > 1 else "bench"
                    fdset = descriptor_pb2.FileDescriptorSet()
                    fdps = [synthetic_fdp(package=pkg)]
                    if b == 0:
                        fdps = ALL_FDPS + fdps
                    fdset.file.extend(fdps)
                    discoverer.load_descriptor_blob(
                        fdset.SerializeToString(), backend_index=b
                    )
            if shard_group is not None:
                from ggrmcp_amd.parallel.dist import sync_discovery

                sync_discovery(discoverer, shard_group, src=0)
            # grpcio channels for the fallback/CPU/streaming paths (grpcio
            # client interoperates with the nghttp2 server)
            for conn in discoverer.connections:
                conn.connect(timeout_s=15)
        else:
            discoverer.connect(timeout_s=30)
            discoverer.discover()
            if shard_group is not None:
                from ggrmcp_amd.parallel.dist import sync_discovery

                sync_discovery(discoverer, shard_group, src=0)

        wire_clients = None
        if args.transport == "native":
            from ggrmcp_amd.backend.native_invoker import NativeWireClient

            wire_clients = [
                NativeWireClient(f"unix:{s}", connections=(
                    args.connections or (16 if args.config == "wide64" else 8)))
                for s in socks
            ]

        bodies = make_bodies(args.config, args.batch, args.payload_bytes, seed=1234 + rank,
                             stream_depth=args.stream_depth, n_backends=n_backends)

        serving = use_gpu and args.config == "hello1k"
        gw = None
        if use_gpu:
            from ggrmcp_amd.engine.batch import GpuPipeline

            pipeline = GpuPipeline(discoverer, cfg, device=dev,
                                   invoke_workers=args.invoke_workers,
                                   wire_clients=wire_clients)

            def step():
                out = pipeline.process_batch(bodies, timeout_s=30.0)
                return out

            if serving:
                # the HEADLINE path: real HTTP through the native gateway
                # (C++ reactors + session guard + GIL-free span executor)
                from ggrmcp_amd.server.native_http import (
                    NativeHTTPGateway,
                    load_module as load_frontend,
                )

                cfg.server.rate_limit_rps = 0  # measurement, not protection
                gw = NativeHTTPGateway(pipeline, discoverer, cfg,
                                       host="127.0.0.1", port=0)
                http_port = gw.start()
                if not gw._span_engines:
                    raise RuntimeError(
                        "native span executor failed to initialize — the "
                        "serving bench must not silently fall back")
                fe_mod = load_frontend()
                client_body = bodies[0].decode()

                def run_clients(requests: int):
                    return fe_mod.bench_client(
                        "127.0.0.1", http_port, args.batch, requests,
                        client_body, args.client_threads)
        else:
            # reference-equivalent CPU plumbing (BASELINE config 1)
            from concurrent.futures import ThreadPoolExecutor

            import ggrmcp_amd.mcp.types as mcp_types  # noqa: F401

            pool = ThreadPoolExecutor(max_workers=args.invoke_workers)
            parsed = []
            for b in bodies:
                d = json.loads(b)
                parsed.append(
                    (d["params"]["name"], json.dumps(d["params"].get("arguments", {})), d["id"])
                )

            def one(item):
                tool, args_json, rid = item
                mi = discoverer.get_method_by_tool(tool)
                if mi.is_server_streaming:
                    chunks = list(
                        discoverer.invoke_streaming(tool, args_json, None, 30.0)
                    )
                    resp = {
                        "jsonrpc": "2.0",
                        "id": rid,
                        "result": {
                            "content": [{"type": "text", "text": c} for c in chunks],
                            "isError": False,
                        },
                    }
                    return json.dumps(resp).encode()
                out = discoverer.invoke_method_by_tool(tool, args_json, None, 30.0)
                resp = {
                    "jsonrpc": "2.0",
                    "id": rid,
                    "result": {
                        "content": [{"type": "text", "text": out}],
                        "isError": False,
                    },
                }
                return json.dumps(resp).encode()

            def step():
                return list(pool.map(one, parsed, chunksize=8))

        def sync():
            if use_gpu:
                torch.cuda.synchronize()
            if dist is not None:
                dist.barrier()

        rtt_p50_ms = rtt_p90_ms = rtt_p99_ms = None
        step_times = []
        if serving:
            # sanity: one real request through the gateway is well-formed
            import http.client as _http

            conn = _http.HTTPConnection("127.0.0.1", http_port, timeout=30)
            conn.request("POST", "/", body=bodies[0],
                         headers={"Content-Type": "application/json"})
            sample = json.loads(conn.getresponse().read())
            conn.close()
            assert sample.get("result", {}).get("isError") is False, sample
            # warmup: every session completes args.warmup requests
            total, _, _, errs = run_clients(args.warmup)
            assert errs == 0, f"warmup client errors: {errs}"
            sync()
            t0 = time.perf_counter()
            total, _, pct, errs = run_clients(args.steps)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            sync()
            assert errs == 0, f"client errors: {errs}"
            assert total == args.batch * args.steps, (total, args.batch,
                                                      args.steps)
            rtt_p50_ms = pct[0] / 1e3
            rtt_p90_ms = pct[1] / 1e3
            rtt_p99_ms = pct[2] / 1e3
        else:
            # warmup
            for _ in range(args.warmup):
                out = step()
            # sanity: responses are well-formed
            sample = json.loads(out[0])
            assert sample.get("result", {}).get("isError") is False, sample

            sync()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                s0 = time.perf_counter()
                out = step()
                step_times.append(time.perf_counter() - s0)
            if use_gpu:
                torch.cuda.synchronize()
            t1 = time.perf_counter()
            sync()

        elapsed = t1 - t0
        # max elapsed across ranks
        if dist is not None:
            t = torch.tensor([elapsed], dtype=torch.float64,
                             device="cuda" if use_gpu and dist.get_backend() == "nccl" else "cpu")
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            elapsed = float(t.item())

        if args.dump_outputs and rank == 0:
            if serving:
                # the load generator counts and discards response bytes, and
                # every session posts the same body at every step, so each
                # step's responses are this body's responses: take them from
                # one more, untimed, step through the same gateway
                out = http_step_responses("127.0.0.1", http_port, bodies[0],
                                          args.batch)
            dump_outputs(args.dump_outputs, out)

        total_requests = args.batch * args.steps * world
        reqs_per_s = total_requests / elapsed
        ms_per_step = elapsed / args.steps * 1e3
        step_p50_ms = (statistics.median(step_times) * 1e3
                       if step_times else None)

        if rank == 0:
            payload_size = args.payload_bytes or {
                "hello1k": 1024, "cpu": 1024, "stream": 1024,
                "multi": 4096, "wide64": 65536,
            }[args.config]
            # config 4 is a MESSAGE-throughput benchmark: report msgs/s as
            # the headline value (the raw stream-open req/s was misleading
            # — 4096 msgs flow per request)
            stream_msgs_s = (reqs_per_s * args.stream_depth
                             if args.config == "stream" else None)
            result = {
                "metric": ("MCP server-streaming msgs/sec (whole node)"
                           if args.config == "stream" else
                           "MCP tool_call→gRPC unary req/sec (whole node)"),
                "value": round(stream_msgs_s if stream_msgs_s is not None
                               else reqs_per_s, 1),
                "unit": "msgs/s" if args.config == "stream" else "req/s",
                "n_gpus": world,
                "steps": args.steps,
                "warmup": args.warmup,
                "ms_per_step": round(ms_per_step, 3),
                "higher_is_better": True,
                "scaling": "weak",
                "vs_baseline": None,
                "dtype": "uint8",
                "data": "synthetic",
            }
            result_cfg = {
                "model": {
                    "hello1k": "hello-service SayHello (HTTP serving)",
                    "pipeline": "hello-service SayHello (batch pipeline)",
                    "cpu": "hello-service SayHello",
                    "wide64": "bench.Wide64 64-field nested proto",
                    "stream": "bench.EchoService/StreamEcho server-streaming",
                    "multi": "4-backend centralized gateway, mixed unary+stream",
                }[args.config],
                "global_batch": args.batch * world,
                "seq_len": payload_size,
                "parallelism": f"dp{world}",
                "mode": ("serving-gpu" if serving
                         else "gpu-pipeline" if use_gpu else "cpu-reference"),
                "sessions": args.batch,
                "payload_bytes": payload_size,
                "backend": f"local grpc over uds, separate process ({args.backend}) x{n_backends}",
                "transport": args.transport,
                "stream_depth": args.stream_depth if args.config == "stream" else None,
                "messages_per_step": (args.batch * args.stream_depth
                                      if args.config == "stream" else None),
            }
            if serving:
                # REAL per-request RTT percentiles from the closed-loop C++
                # client (one request in flight per session)
                result_cfg["p50_rtt_ms"] = round(rtt_p50_ms, 3)
                result_cfg["p90_rtt_ms"] = round(rtt_p90_ms, 3)
                result_cfg["p99_rtt_ms"] = round(rtt_p99_ms, 3)
                result_cfg["http"] = "native frontend, C++ closed-loop client"
            elif step_p50_ms is not None:
                # batch-step wall-time median — NOT a request RTT
                result_cfg["ms_per_step_p50"] = round(step_p50_ms, 3)
            result["config"] = result_cfg
            if serving:
                result["config"]["engine_stats"] = gw._fe.native_stats()
                result["config"]["pipeline_stats"] = (
                    pipeline.engine.stats.snapshot())
            elif use_gpu:
                result["config"]["engine_stats"] = pipeline.engine.stats.snapshot()
            print(json.dumps(result), flush=True)
    finally:
        if gw is not None:
            gw.stop()
        for bp in backend_procs:
            bp.terminate()
        for bp in backend_procs:
            try:
                bp.wait(timeout=5)
            except Exception:
                bp.kill()
        for s in socks:
            if os.path.exists(s):
                os.unlink(s)
        if dist is not None:
            dist.destroy_process_group()


if __name__ == "__main__":
    main()
