"""Flagship benchmark: streaming WordCount throughput (events/sec, whole node).

BASELINE.md headline: pathway's published WordCount figure is 2,000,000
messages/s with p95 end-to-end latency < 50 ms (4 CPU cores/system,
docs/.../50.how-live-data-framework-connectors-work.md:276).  This bench
runs the same shape — a stream of words → incremental groupby(word).count
→ consolidated output deltas — through the pathway_amd GPU engine, with
the WHOLE-NODE ingest path billed inside the timed region: newline-
separated wire bytes start in pinned HOST memory, are DMA'd H2D on a
dedicated copy stream (double-buffered to overlap with compute), parsed
(newline scan), token-hashed (HIP varlen xxh128 kernel), dictionary-
decoded (sorted-pool binary-search kernel), keyed, shuffled by key shard
(RCCL all-to-all over xGMI for N>1), segment-reduced and merged into
GPU-resident state; the (-old,+new) count deltas are emitted.

Driver contract: --gpus N --steps K --warmup W; launched via torchrun for
N>1 (one rank per GPU, RCCL); rank 0 prints ONE json line.

A plain run does only what the headline figure needs: set up, warm up,
time the K steps, print the line.  --dump-outputs DIR additionally writes
the output deltas of the last timed step as DIR/<name>.npy (inputs are
seeded, so two builds can be compared array for array).  --full adds the
p50 RAG latency probe (config.rag_*), which takes a run of its own.
"""

from __future__ import annotations

import argparse
import json
import os
import time

import torch


def measure_rag_p50(device, *, n_docs: int = 100_000, n_queries: int = 128,
                    qps: float = 200.0) -> dict:
    """p50 RAG query latency at fixed QPS (the second half of the
    BASELINE metric): bge-small-geometry embedder (bf16, hipGraph) +
    KNN top-20 + cosine rerank to top-5 over synthetic docs.

    Each query is timed end-to-end (tokenize -> embed -> search ->
    rerank) while being issued on a fixed-interval schedule."""
    import numpy as np
    import time as _time

    from pathway_amd.engine.ann import IvfFlatState
    from pathway_amd.xpacks.llm._encoder import get_encoder

    enc = get_encoder(device=device)
    rng = np.random.default_rng(7)
    vocab = [f"term{i}" for i in range(5000)]
    docs = [
        " ".join(rng.choice(vocab, size=12)) for _ in range(2048)
    ]
    # doc embeddings: embed a representative set, then tile with noise to
    # n_docs (index scale is what matters; embedding all n_docs would
    # measure the embedder, which the wordcount half already covers)
    base = torch.stack(
        [torch.from_numpy(np.asarray(e)) for e in enc.encode(docs, batch_size=1024)]
    ).to(device)
    reps = (n_docs + base.shape[0] - 1) // base.shape[0]
    vecs = base.repeat(reps, 1)[:n_docs]
    vecs = vecs + 0.01 * torch.randn(
        vecs.shape, device=vecs.device, dtype=vecs.dtype
    )
    keys = torch.stack([
        torch.arange(1, n_docs + 1, dtype=torch.int64, device=device),
        torch.zeros(n_docs, dtype=torch.int64, device=device),
    ], dim=1)
    index = IvfFlatState(device, "cos")
    index.update(keys, vecs.float(), torch.ones(n_docs, dtype=torch.int64, device=device))

    queries = [" ".join(rng.choice(vocab, size=8)) for _ in range(n_queries)]

    def serve_one(q: str) -> None:
        emb = enc.encode([q], batch_size=1)[0]
        qv = torch.from_numpy(np.asarray(emb)).to(device).reshape(1, -1)
        ids, scores, valid = index.search(qv.float(), 20)
        # rerank: exact cosine over the top-20 candidates -> top-5
        cand = ids[0, :, 0].clamp(min=1) - 1
        cvecs = vecs.index_select(0, cand)
        sc = torch.nn.functional.normalize(qv.float(), dim=1) @ torch.nn.functional.normalize(cvecs.float(), dim=1).T
        torch.topk(sc[0], min(5, sc.shape[1]))
        torch.cuda.synchronize(device)

    for q in queries[:8]:  # warmup (graph capture etc.)
        serve_one(q)
    interval = 1.0 / qps
    lat = []
    next_t = _time.perf_counter()
    for q in queries:
        now = _time.perf_counter()
        if now < next_t:
            _time.sleep(next_t - now)
        t0 = _time.perf_counter()
        serve_one(q)
        lat.append((_time.perf_counter() - t0) * 1000.0)
        next_t += interval
    lat.sort()
    return {
        "rag_p50_ms": lat[len(lat) // 2],
        "rag_p95_ms": lat[max(0, int(len(lat) * 0.95) - 1)],
        "rag_qps": qps,
        "rag_docs": n_docs,
        "rag_queries": n_queries,
    }


DUMP_BYTE_CAP = 64 * 1024 * 1024


def _int_words(t: torch.Tensor) -> torch.Tensor:
    """int64 (n, ...) -> float64 (n, ..., 2) of (high, low) unsigned 32-bit
    words: exact in float64, unlike a direct cast of a 64-bit hash."""
    t = t.to(torch.int64).cpu()
    hi = (t >> 32) & 0xFFFFFFFF
    lo = t & 0xFFFFFFFF
    return torch.stack([hi, lo], dim=-1).to(torch.float64).reshape(t.shape[0], -1)


def dump_outputs(out_dir: str, batches: list, suffix: str = "") -> None:
    """Write the deltas the sink received in the last timed step.

    One float64 array per field, rows in the order the writer got them:
      keys   (n, 4)  128-bit row key as four 32-bit words
      diffs  (n,)    -1 retraction / +1 insertion
      word   (n,)    dictionary code of the word (index into the vocab)
      count  (n,)    the new (or retracted) count
    Above DUMP_BYTE_CAP in total, a fixed seeded sample of the rows is kept
    (same rows in every run with the same arguments).  With several ranks
    each writes its own shard as <name><suffix>.npy."""
    import numpy as np

    from pathway_amd.engine.batch import DeltaBatch
    from pathway_amd.engine.column import PointerColumn, StringColumn, TensorColumn

    assert batches, "--dump-outputs: the timed path emitted nothing in its last step"
    b = DeltaBatch.concat(batches)
    arrays = {
        "keys": _int_words(b.keys),
        "diffs": b.diffs.cpu().to(torch.float64),
    }
    for name, col in b.columns.items():
        if isinstance(col, StringColumn):
            arrays[name] = col.codes.cpu().to(torch.float64)
        elif isinstance(col, PointerColumn):
            arrays[name] = _int_words(col.pairs)
        elif isinstance(col, TensorColumn):
            arrays[name] = col.tensor.cpu().to(torch.float64)
        else:
            raise TypeError(f"--dump-outputs: cannot dump column {name!r} ({type(col).__name__})")
    n = len(b)
    row_bytes = sum(a[0].numel() * 8 for a in arrays.values()) if n else 0
    if n * row_bytes > DUMP_BYTE_CAP:
        keep = DUMP_BYTE_CAP // row_bytes
        idx = np.sort(np.random.default_rng(2024).choice(n, size=keep, replace=False))
        sel = torch.from_numpy(idx)
        arrays = {k: a.index_select(0, sel) for k, a in arrays.items()}
    os.makedirs(out_dir, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, f"{name}{suffix}.npy"), a.numpy())


def main() -> None:
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument(
        "--batch",
        type=int,
        default=None,
        help="events per step per GPU (default 4M on GPU, 100k on CPU)",
    )
    p.add_argument("--vocab", type=int, default=50_000)
    p.add_argument("--device", type=str, default=None)
    p.add_argument(
        "--ingest",
        choices=["codes", "bytes"],
        default="bytes",
        help="codes: pre-parsed dictionary codes; bytes: raw newline-separated "
        "byte stream tokenized+hashed on-device (HIP varlen kernel)",
    )
    p.add_argument(
        "--dump-outputs",
        metavar="DIR",
        default=None,
        help="after the timed steps, write the last step's output deltas "
        "as DIR/<name>.npy (float64)",
    )
    p.add_argument(
        "--full",
        action="store_true",
        help="also run the p50 RAG query latency probe (config.rag_*)",
    )
    args = p.parse_args()

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))

    use_cuda = torch.cuda.is_available()
    if args.device:
        device = torch.device(args.device)
    elif use_cuda:
        device = torch.device(f"cuda:{local_rank % torch.cuda.device_count()}")
    else:
        device = torch.device("cpu")
    if use_cuda:
        torch.cuda.set_device(device)

    os.environ["PW_DEVICE"] = str(device)
    if args.batch is None:
        args.batch = 4_000_000 if use_cuda else 100_000

    import numpy as np

    import pathway_amd as pw
    import pathway_amd.parallel as par
    from pathway_amd.engine import hashing
    from pathway_amd.engine.batch import DeltaBatch
    from pathway_amd.engine.column import GLOBAL_STRING_POOL, StringColumn
    from pathway_amd.engine.nodes import InputNode
    from pathway_amd.engine.runtime import OutputNode, Runtime
    from pathway_amd.internals import dtype as dt
    from pathway_amd.internals.api import TAG_INT
    from pathway_amd.internals.table import Table
    from pathway_amd.internals.universe import Universe

    comm = None
    if world > 1:
        backend = os.environ.get("PW_BACKEND") or ("nccl" if use_cuda else "gloo")
        comm = par.init(backend=backend, device=device)

    # ---- synthetic parsed word stream (identical vocab on all ranks) ----
    # fixed word width: zero-pad to however many digits the vocab needs
    DIG = max(6, len(str(args.vocab - 1)))
    WW = 4 + DIG  # b"word" + digits
    vocab = [f"word{i:0{DIG}d}" for i in range(args.vocab)]
    GLOBAL_STRING_POOL.codes(vocab)
    GLOBAL_STRING_POOL.synchronized = True
    GLOBAL_STRING_POOL.hash_tensors(device)  # pre-stage pool hashes in HBM

    # synthetic stream RNG lives ON DEVICE: a real connector DMAs messages
    # into HBM; generating on host and copying would bill a host artifact
    # to the engine. Per-rank independent streams via distinct seeds.
    gen = torch.Generator(device=device if use_cuda else "cpu")
    gen.manual_seed(1234 + rank)

    class WordStream:
        """Source: per pull, one micro-batch of `batch` word events."""

        def __init__(self, batch: int, vocab_n: int):
            self.batch = batch
            self.vocab_n = vocab_n
            self.counter = 0

        def next_time(self):
            return None  # driven manually by the bench loop

        def pull(self, t, dev):
            n = self.batch
            codes = torch.randint(
                0, self.vocab_n, (n,), dtype=torch.int64, generator=gen,
                device=gen.device,
            ).to(dev, non_blocking=True)
            seq = torch.arange(
                self.counter, self.counter + n, dtype=torch.int64, device=dev
            )
            self.counter += n
            klo, khi = hashing.value_hash_words(seq, TAG_INT)
            keys = torch.stack([klo, khi], dim=1)
            cols = {"word": StringColumn(codes, GLOBAL_STRING_POOL, dt.STR)}
            diffs = torch.ones(n, dtype=torch.int64, device=dev)
            return DeltaBatch(keys, cols, diffs, t)

        def reset(self):
            self.counter = 0

    class HostByteStream:
        """Honest whole-node ingest.

        The word stream exists as newline-separated BYTES IN HOST MEMORY
        (pinned staging buffers — the analog of a socket / page-cache
        buffer a real connector reads from; like the reference harness's
        pre-created 5M-row input, the wire bytes are synthesized before
        the timed region).  Every timed step then performs the full
        connector pipeline:

          H2D DMA (hipMemcpyAsync on a dedicated copy stream,
          double-buffered so copy overlaps the previous step's compute)
          -> newline scan -> varlen xxh128 token hash (HIP kernel)
          -> dictionary lookup (sorted-pool binary-search HIP kernel)
          -> keyed DeltaBatch.

        The output `word` column is DERIVED FROM THE PARSED BYTES via the
        dictionary lookup; the codes used to synthesize the wire buffer
        never enter the engine.  PCIe bytes are billed inside the timed
        region (batch*(WW+1) bytes per step per GPU).
        """

        def __init__(self, batch: int, vocab_n: int, pool_buffers: int = 6):
            self.batch = batch
            self.vocab_n = vocab_n
            self.counter = 0
            self.nbytes = batch * (WW + 1)
            # ---- host wire buffers (the "input stream"), pinned ----
            vb = np.frombuffer(
                "".join(vocab).encode(), dtype=np.uint8
            ).reshape(vocab_n, WW)
            rng = np.random.default_rng(1234 + rank)
            self.host_bufs = []
            for _ in range(pool_buffers):
                codes = rng.integers(0, vocab_n, size=batch)
                msg = np.empty((batch, WW + 1), dtype=np.uint8)
                msg[:, :WW] = vb[codes]
                msg[:, WW] = 10  # newline
                tbuf = torch.from_numpy(msg.reshape(-1))
                if use_cuda:
                    tbuf = tbuf.pin_memory()
                self.host_bufs.append(tbuf)
            # ---- device dictionary: open-addressing hash table ----
            # pool code == row index in the pool hash tensors, so the
            # identity-valued table maps token hash -> code in O(1)
            plo, phi = GLOBAL_STRING_POOL.hash_tensors(device)
            if use_cuda:
                from pathway_amd import ops

                self.dict_ht = ops.DeviceHashTable(plo, phi)
            self.miss = torch.zeros((), dtype=torch.int64, device=device)
            # ---- double-buffered staging ----
            if use_cuda:
                self.copy_stream = torch.cuda.Stream(device)
                self.staged = [
                    torch.empty(self.nbytes, dtype=torch.uint8, device=device)
                    for _ in range(2)
                ]
                self.ready = [torch.cuda.Event(), torch.cuda.Event()]
                self.free = [torch.cuda.Event(), torch.cuda.Event()]
                for ev in self.free:
                    ev.record()  # both slots initially writable
                self.next_buf = 0
                self.cur = 0
                self._prefetch(0)

        def _prefetch(self, slot: int) -> None:
            """Issue async H2D of the next host buffer into `slot`."""
            with torch.cuda.stream(self.copy_stream):
                self.copy_stream.wait_event(self.free[slot])
                self.staged[slot].copy_(
                    self.host_bufs[self.next_buf], non_blocking=True
                )
                self.ready[slot].record(self.copy_stream)
            self.next_buf = (self.next_buf + 1) % len(self.host_bufs)

        def next_time(self):
            return None

        def pull(self, t, dev):
            from pathway_amd.engine.column import PointerColumn
            from pathway_amd.internals.api import TAG_STR

            n = self.batch
            if dev.type == "cuda":
                from pathway_amd import ops

                cur = self.cur
                torch.cuda.current_stream().wait_event(self.ready[cur])
                buf = self.staged[cur]
                # PARSE on device: newline scan -> token [start, end) spans
                # (pw_scan_positions: ordered match positions, count+emit)
                nl = ops.scan_positions_gpu(buf, 10)
                starts = torch.cat(
                    [torch.zeros(1, dtype=torch.int64, device=dev), nl[:-1] + 1]
                )
                ends = nl
                glo, ghi = ops.varlen_hash_se_gpu(buf, starts, ends, TAG_STR)
                # word column derived from the parsed bytes: dictionary
                # probe of the token hash in the device hash table (codes
                # are -1 on miss already)
                codes, found = self.dict_ht.probe(glo, ghi)
                self.miss += (~found).sum()
                # this step's reads of `buf` are enqueued; allow the copy
                # stream to overwrite the slot for step t+2
                self.free[cur].record()
                self.cur = 1 - cur
                self._prefetch(1 - cur)  # overlaps with this step's compute
            else:
                # CPU fallback (not the measured path): numpy parse of the
                # same wire buffer -> dictionary-encode via the string pool
                raw = self.host_bufs[self.counter // n % len(self.host_bufs)]
                msg = np.ascontiguousarray(
                    raw.numpy().reshape(n, WW + 1)[:, :WW]
                )
                toks = msg.view(f"S{WW}").ravel()
                words_l = [t_.decode() for t_ in toks]
                codes_np = GLOBAL_STRING_POOL.codes(words_l)
                codes = torch.from_numpy(codes_np)
                plo, phi = GLOBAL_STRING_POOL.hash_tensors(dev)
                glo = plo.index_select(0, codes)
                ghi = phi.index_select(0, codes)
            seq = torch.arange(
                self.counter, self.counter + n, dtype=torch.int64, device=dev
            )
            self.counter += n
            klo, khi = hashing.value_hash_words(seq, TAG_INT)
            keys = torch.stack([klo, khi], dim=1)
            cols = {
                "word": StringColumn(codes, GLOBAL_STRING_POOL, dt.STR),
                "wkey": PointerColumn(torch.stack([glo, ghi], dim=1)),
            }
            diffs = torch.ones(n, dtype=torch.int64, device=dev)
            return DeltaBatch(keys, cols, diffs, t)

        def reset(self):
            self.counter = 0

    if args.ingest == "bytes":
        source = HostByteStream(args.batch, args.vocab)
        in_node = InputNode(source, device)
        words = Table(
            in_node, {"word": dt.STR, "wkey": dt.POINTER}, Universe()
        )
        counts = words.groupby(pw.this.word, id=pw.this.wkey).reduce(
            pw.this.word, count=pw.reducers.count()
        )
    else:
        source = WordStream(args.batch, args.vocab)
        in_node = InputNode(source, device)
        words = Table(in_node, {"word": dt.STR}, Universe())
        counts = words.groupby(pw.this.word).reduce(
            pw.this.word, count=pw.reducers.count()
        )

    emitted = [0]
    last_out: list = []  # batches delivered at the most recent timestamp

    def counting_writer(batch):
        emitted[0] += len(batch)
        if last_out and last_out[0].time != batch.time:
            last_out.clear()
        last_out.append(batch)

    sink = OutputNode(counts._node, counting_writer, device)
    rt = Runtime([sink], device=device, comm=comm)

    def sync():
        if use_cuda:
            torch.cuda.synchronize(device)

    def barrier():
        if comm is not None:
            comm.barrier()

    # ---- warmup ----
    t = 0
    for _ in range(args.warmup):
        rt.step_once(t)
        t += 2  # even timestamps (reference alt-neu convention)
    sync()
    barrier()
    sync()

    if os.environ.get("PW_TORCH_PROF"):
        # host/device breakdown of the steady-state step (diagnostics only)
        from torch.profiler import ProfilerActivity, profile

        acts = [ProfilerActivity.CPU]
        if use_cuda:
            acts.append(ProfilerActivity.CUDA)
        with profile(activities=acts) as prof:
            for _ in range(3):
                rt.step_once(t)
                t += 2
            sync()
        ka = prof.key_averages()
        print(ka.table(sort_by="self_cpu_time_total", row_limit=30))
        if use_cuda:
            print(ka.table(sort_by="self_cuda_time_total", row_limit=20))

    # ---- timed region: exactly K steps ----
    step_times = []
    t0 = time.perf_counter()
    for _ in range(args.steps):
        s0 = time.perf_counter()
        rt.step_once(t)
        t += 2
        sync()
        step_times.append(time.perf_counter() - s0)
    sync()
    barrier()
    sync()
    elapsed = time.perf_counter() - t0

    # max over ranks
    if comm is not None:
        import torch.distributed as dist

        et = torch.tensor([elapsed], dtype=torch.float64, device=comm._comm_device)
        dist.all_reduce(et, op=dist.ReduceOp.MAX)
        elapsed = float(et.item())

    if args.dump_outputs:
        dump_outputs(
            args.dump_outputs,
            [b for b in last_out if b.time == t - 2] if args.steps > 0 else [],
            suffix=f"_rank{rank}" if world > 1 else "",
        )

    # second half of the BASELINE metric: p50 RAG latency at fixed QPS
    # (--full only; measured on rank 0 after the timed wordcount region;
    # single GPU)
    rag_stats: dict = {}
    if (
        args.full
        and use_cuda
        and rank == 0
        and not os.environ.get("PW_NO_RAG_BENCH")
    ):
        try:
            rag_stats = measure_rag_p50(device)
        except Exception as e:  # never fail the headline on the rag probe
            rag_stats = {"rag_error": str(e)[:200]}

    n_gpus = world if world > 1 else 1
    total_events = args.batch * args.steps * n_gpus
    value = total_events / elapsed
    ms_per_step = elapsed / args.steps * 1000.0
    p95 = sorted(step_times)[max(0, int(len(step_times) * 0.95) - 1)] * 1000.0

    if rank == 0:
        print(
            json.dumps(
                {
                    # BASELINE.json metric; `value` is the events/s half,
                    # config.rag_p50_ms carries the latency half
                    "metric": "events/sec (whole node) on WordCount stream + p50 RAG query latency at fixed QPS",
                    "value": value,
                    "unit": "events/s",
                    "n_gpus": n_gpus,
                    "steps": args.steps,
                    "warmup": args.warmup,
                    "ms_per_step": ms_per_step,
                    "higher_is_better": True,
                    "scaling": "weak",
                    "vs_baseline": value / 2_000_000.0,
                    "dtype": "int64/string-dict",
                    "data": "synthetic",
                    "config": {
                        "model": "wordcount: stream -> groupby(word).count -> output deltas",
                        "global_batch": args.batch * n_gpus,
                        "seq_len": 1,
                        "parallelism": f"dp{n_gpus} (shard exchange: RCCL all-to-all)",
                        "vocab": args.vocab,
                        "ingest": args.ingest,
                        "p95_step_latency_ms": p95,
                        "emitted_delta_rows": emitted[0],
                        "h2d_bytes_per_step": (
                            source.nbytes if args.ingest == "bytes" else 0
                        ),
                        "dict_misses": (
                            int(source.miss.item())
                            if args.ingest == "bytes" and use_cuda
                            else 0
                        ),
                        **rag_stats,
                    },
                }
            )
        )

    if comm is not None:
        import torch.distributed as dist

        dist.destroy_process_group()


if __name__ == "__main__":
    main()
