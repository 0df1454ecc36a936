"""Run configuration (reference internals/config.py:65-140 behavior).

Environment variables:
  PATHWAY_THREADS / PATHWAY_PROCESSES — worker counts (reference semantics)
  PW_DEVICE — engine device override ("cpu", "cuda", "cuda:0", ...)
  PW_BM25 — BM25 index state override for A/B runs: "host" (numpy CSR,
    float64, one query at a time) or "device" (CSR postings on the node's
    device, batched pw_bm25_score kernel, float32).  Unset: device on a
    GPU node, host on a CPU node.  Read when the index node is built
    (stdlib/indexing/bm25.py).
  PW_INGEST — pw.io.plaintext.read path override: "host" (python lines
    through StringPool.codes) or "device" (file bytes to the device,
    newline scan, unseen lines interned there by the pool's
    DeviceDictionary; on a CPU node its numpy fallback).  Unset: device on
    a GPU node with the native library, host otherwise.  A read with a
    file that holds a carriage return or invalid UTF-8 takes the host path
    as a whole, so its rows and exceptions stay what they were.  Read when
    the reader is built (engine/ingest_device.py).
On GPU hosts the engine defaults to cuda (one worker per GPU, RCCL
exchange); in CPU-only containers it runs on torch-cpu tensors.
"""

from __future__ import annotations

import os
from dataclasses import dataclass, field


@dataclass
class PathwayConfig:
    device: str | None = None
    ignore_asserts: bool = bool(os.environ.get("PATHWAY_IGNORE_ASSERTS"))
    terminate_on_error: bool = True
    runtime_typechecking: bool = False
    license_key: str | None = os.environ.get("PATHWAY_LICENSE_KEY")
    monitoring_server: str | None = None
    detailed_metrics_dir: str | None = None
    process_id: int = int(os.environ.get("PATHWAY_PROCESS_ID", "0"))
    processes: int = int(os.environ.get("PATHWAY_PROCESSES", "1"))
    threads: int = int(os.environ.get("PATHWAY_THREADS", "1"))

    def resolve_device(self) -> str:
        if self.device is not None:
            return self.device
        env = os.environ.get("PW_DEVICE")
        if env:
            return env
        try:
            import torch

            if torch.cuda.is_available():
                local_rank = int(os.environ.get("LOCAL_RANK", "0"))
                return f"cuda:{local_rank % max(torch.cuda.device_count(), 1)}"
        except Exception:
            pass
        return "cpu"


pathway_config = PathwayConfig()


def set_device(device: str | None) -> None:
    pathway_config.device = device


def get_device() -> str:
    return pathway_config.resolve_device()


def set_license_key(key: str | None) -> None:
    pathway_config.license_key = key


def set_monitoring_config(*, server_endpoint: str | None = None,
                          detailed_metrics_dir: str | None = None,
                          **kwargs) -> None:
    pathway_config.monitoring_server = server_endpoint
    pathway_config.detailed_metrics_dir = detailed_metrics_dir
