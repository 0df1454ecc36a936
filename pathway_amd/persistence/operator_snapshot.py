"""Operator snapshots (reference persistence/operator_snapshot.rs:21-380 +
engine/dataflow/persist.rs maybe_persist).

Stateful nodes expose save_state()/load_state(); the Runtime snapshots
every node's state at commit boundaries (PersistenceMode.OPERATOR_PERSISTING)
so recovery restores operator state directly instead of replaying input
snapshots.  Serialization is host-side (tensors → numpy, dictionary
strings decoded — pool codes are process-local) with zlib compression.
"""

from __future__ import annotations

import os
import pickle
import zlib
from typing import Any

import numpy as np
import torch


def column_to_portable(col) -> dict:
    from pathway_amd.engine.column import (
        ObjectColumn,
        PointerColumn,
        StringColumn,
        TensorColumn,
    )

    if isinstance(col, TensorColumn):
        return {
            "kind": "tensor",
            "data": col.tensor.cpu().numpy(),
            "mask": col.mask.cpu().numpy() if col.mask is not None else None,
            "dtype": col.dtype,
        }
    if isinstance(col, PointerColumn):
        return {"kind": "pointer", "data": col.pairs.cpu().numpy(), "dtype": col.dtype}
    if isinstance(col, StringColumn):
        return {"kind": "string", "data": col.to_pylist(), "dtype": col.dtype}
    if isinstance(col, ObjectColumn):
        return {"kind": "object", "data": list(col.values), "dtype": col.dtype}
    raise TypeError(f"unsnapshotable column {type(col)}")


def column_from_portable(d: dict, device):
    from pathway_amd.engine.column import (
        ObjectColumn,
        PointerColumn,
        StringColumn,
        TensorColumn,
        obj_array,
    )

    kind = d["kind"]
    if kind == "tensor":
        t = torch.from_numpy(np.ascontiguousarray(d["data"])).to(device)
        mask = (
            torch.from_numpy(np.ascontiguousarray(d["mask"])).to(device)
            if d["mask"] is not None
            else None
        )
        return TensorColumn(t, d["dtype"], mask)
    if kind == "pointer":
        return PointerColumn(
            torch.from_numpy(np.ascontiguousarray(d["data"])).to(device), d["dtype"]
        )
    if kind == "string":
        return StringColumn.from_strings(d["data"], device=device)
    if kind == "object":
        return ObjectColumn(obj_array(d["data"]), d["dtype"])
    raise TypeError(kind)


def tensor_to_portable(t: torch.Tensor):
    return t.cpu().numpy()


def tensor_from_portable(a, device) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


class _RestrictedUnpickler(pickle.Unpickler):
    """Allowlisting unpickler: operator snapshots are numpy/dtype/builtin
    structures only — a writable persistence root must not allow code
    execution on restart (ADVICE r1 finding 5)."""

    _ALLOWED = {
        ("builtins", None),  # module allowed, names checked below
        ("numpy", None),
        ("numpy.core.multiarray", None),
        ("numpy._core.multiarray", None),
        ("numpy.dtypes", None),
        ("collections", None),
        ("pathway_amd.internals.dtype", None),
        ("pathway_amd.internals.api", None),
        ("pathway_amd.internals.json", None),
        ("pathway_amd.internals.datetime_types", None),
        ("pandas._libs.tslibs.timestamps", None),
        ("pandas._libs.tslibs.timedeltas", None),
        ("datetime", None),
        ("_codecs", None),
    }
    _DENY_NAMES = {"eval", "exec", "compile", "open", "__import__", "getattr",
                   "setattr", "delattr", "input", "breakpoint"}

    def find_class(self, module, name):
        top = module.split(".")[0]
        roots = {m.split(".")[0] for m, _ in self._ALLOWED}
        if top not in roots or name in self._DENY_NAMES:
            raise pickle.UnpicklingError(
                f"operator snapshot references disallowed global "
                f"{module}.{name}"
            )
        return super().find_class(module, name)


def _safe_loads(data: bytes):
    import io as _io

    return _RestrictedUnpickler(_io.BytesIO(data)).load()


class OperatorSnapshotStore:
    """Operator-state snapshots over a persistence BlobStore.

    Writes run on a background thread (the reference's background
    snapshot writer/merger, operator_snapshot.rs:172-380 — amortization
    here is by not blocking the step loop; state is full-serialize since
    the engine's per-node states are already consolidated tensors).
    Two rotations are kept; load takes the newest readable one.
    """

    def __init__(self, root: str):
        from pathway_amd.persistence.backends import FileStore

        self.store = FileStore(root)
        self.prefix = "operator_snapshots/0"
        self._init_common()

    @classmethod
    def over_store(cls, store, worker: int) -> "OperatorSnapshotStore":
        self = cls.__new__(cls)
        self.store = store
        self.prefix = f"operator_snapshots/{worker}"
        self._init_common()
        return self

    def _init_common(self):
        import threading

        self._seq = 0
        self._thread = None
        self._lock = threading.Lock()

    def _write(self, payload: bytes, seq: int) -> None:
        self.store.put(f"{self.prefix}/snapshot-{seq}.bin", payload)
        # keep the last two rotations
        keys = sorted(
            self.store.list(self.prefix + "/"),
            key=lambda k: int(k.rsplit("-", 1)[-1].split(".")[0]),
        )
        for k in keys[:-2]:
            self.store.delete(k)

    def save(self, snapshot_time: int, states: dict[str, Any]) -> None:
        payload = zlib.compress(
            pickle.dumps({"time": snapshot_time, "states": states}, protocol=4), 1
        )
        with self._lock:
            seq = self._seq
            self._seq += 1
            if self._thread is not None:
                self._thread.join()
            import threading

            self._thread = threading.Thread(
                target=self._write, args=(payload, seq), daemon=True
            )
            self._thread.start()

    def wait(self) -> None:
        with self._lock:
            if self._thread is not None:
                self._thread.join()
                self._thread = None

    def load(self) -> tuple[int, dict[str, Any]] | None:
        self.wait()
        keys = sorted(
            self.store.list(self.prefix + "/"),
            key=lambda k: int(k.rsplit("-", 1)[-1].split(".")[0]),
        )
        for key in reversed(keys):
            data = self.store.get(key)
            if not data:
                continue
            try:
                d = _safe_loads(zlib.decompress(data))
                return d["time"], d["states"]
            except Exception:
                continue  # fall back to the previous rotation
        return None


# ------------------------------------------------- node state dispatchers --

def _arrangement_to_portable(arr) -> dict | None:
    if arr is None:
        return None
    return {
        "key_words": [tensor_to_portable(w) for w in arr.key_words],
        "vhash_words": [tensor_to_portable(w) for w in arr.vhash_words],
        "weights": tensor_to_portable(arr.weights),
        "columns": {n: column_to_portable(c) for n, c in arr.columns.items()},
    }


def _arrangement_from_portable(d, device):
    if d is None:
        return None
    from pathway_amd.engine.state import Arrangement

    cols = {n: column_from_portable(c, device) for n, c in d["columns"].items()}
    arr = Arrangement(device, cols)
    arr.key_words = [tensor_from_portable(w, device) for w in d["key_words"]]
    arr.vhash_words = [tensor_from_portable(w, device) for w in d["vhash_words"]]
    arr.weights = tensor_from_portable(d["weights"], device)
    arr.columns = cols
    return arr


def _sidestore_to_portable(store) -> dict:
    spine = getattr(store, "spine", None)
    if spine is None:
        return {"levels": None}
    return {
        "levels": [_arrangement_to_portable(l) for l in spine.levels],
        "protos": {n: column_to_portable(c.take(
            __import__("torch").zeros(0, dtype=__import__("torch").int64)
        )) for n, c in spine.protos.items()} if spine.protos else {},
    }


def _sidestore_from_portable(d, device):
    from pathway_amd.engine.nodes_join import _SideStore
    from pathway_amd.engine.state import SpineArrangement

    st = _SideStore(device)
    if d.get("levels") is None:
        return st
    levels = [_arrangement_from_portable(l, device) for l in d["levels"]]
    protos = (
        levels[0].columns
        if levels
        else {n: column_from_portable(c, device) for n, c in d.get("protos", {}).items()}
    )
    sp = SpineArrangement(device, protos)
    sp.levels = [l for l in levels if l is not None]
    st.spine = sp
    return st


def _batch_to_portable(b) -> dict:
    return {
        "keys": tensor_to_portable(b.keys),
        "diffs": tensor_to_portable(b.diffs),
        "time": b.time,
        "columns": {n: column_to_portable(c) for n, c in b.columns.items()},
    }


def _batch_from_portable(d, device):
    from pathway_amd.engine.batch import DeltaBatch

    return DeltaBatch(
        tensor_from_portable(d["keys"], device),
        {n: column_from_portable(c, device) for n, c in d["columns"].items()},
        tensor_from_portable(d["diffs"], device),
        d["time"],
    )


def node_state_save(node):
    """Portable state of a stateful node, or None (reference maybe_persist,
    persist.rs:679)."""
    from pathway_amd.engine.nodes import GroupReduceNode
    from pathway_amd.engine.nodes_dedup import DeduplicateNode
    from pathway_amd.engine.nodes_index import ExternalIndexNode
    from pathway_amd.engine.nodes_join import JoinNode, KeyedMergeNode, SemiJoinNode
    from pathway_amd.engine.nodes_recompute import RecomputeNode
    from pathway_amd.engine.nodes_temporal import BufferNode, ForgetNode, FreezeNode

    if isinstance(node, GroupReduceNode):
        return {
            "kind": "reduce",
            "seq": node.seq,
            "add_keys": [tensor_to_portable(w) for w in node.add_keys]
            if node.add_keys is not None
            else None,
            "add_accs": {n: tensor_to_portable(t) for n, t in node.add_accs.items()},
            "add_carried": {
                n: column_to_portable(c) for n, c in node.add_carried.items()
            },
            "multiset": _arrangement_to_portable(node.multiset_store),
        }
    if isinstance(node, JoinNode) or isinstance(node, KeyedMergeNode):
        return {
            "kind": "two_store",
            "l": _sidestore_to_portable(node.lstore),
            "r": _sidestore_to_portable(node.rstore),
        }
    if isinstance(node, SemiJoinNode):
        return {
            "kind": "semi",
            "l": _sidestore_to_portable(node.lstore),
            "r": _sidestore_to_portable(node.rcount),
        }
    if isinstance(node, DeduplicateNode):
        return {"kind": "dedup", "state": node.state}
    if isinstance(node, RecomputeNode):
        return {
            "kind": "recompute",
            "stores": [_sidestore_to_portable(s) for s in node.stores],
            "prev": node.prev_output,
        }
    if isinstance(node, BufferNode):
        return {
            "kind": "buffer",
            "wm": node.watermark,
            "held": [
                (_batch_to_portable(b), tensor_to_portable(t)) for b, t in node.held
            ],
        }
    if isinstance(node, ForgetNode):
        return {
            "kind": "forget",
            "wm": node.watermark,
            "live": [
                (_batch_to_portable(b), tensor_to_portable(t)) for b, t in node.live
            ],
        }
    if isinstance(node, FreezeNode):
        return {"kind": "freeze", "wm": node.watermark}
    if isinstance(node, ExternalIndexNode):
        st = node.state
        return {
            "kind": "vindex",
            "keys": tensor_to_portable(st.keys),
            "vectors": tensor_to_portable(st.vectors) if st.vectors is not None else None,
            "payload": st.payload,
            "answers": node.answers,
        }
    if type(node).__name__ == "_BM25IndexNode":
        return {"kind": "bm25", "state": node.state, "answers": node.answers}
    from pathway_amd.engine.nodes_asof import AsofJoinNode

    if isinstance(node, AsofJoinNode):
        return {
            "kind": "asof",
            "l": _asof_side_to_portable(node.L),
            "r": _asof_side_to_portable(node.R),
        }
    from pathway_amd.engine.nodes_session import SessionAssignNode
    from pathway_amd.engine.nodes_sort import SortPrevNextNode

    if isinstance(node, (SessionAssignNode, SortPrevNextNode)):
        return {"kind": "sorted_side", "s": _asof_side_to_portable(node.S)}
    return None


def _asof_side_to_portable(S):
    return {
        "words": [tensor_to_portable(w) for w in S.words],
        "weights": tensor_to_portable(S.weights),
        "cols": {n: column_to_portable(c) for n, c in S.cols.items()}
        if S.cols is not None
        else None,
    }


def _asof_side_from_portable(d, device):
    from pathway_amd.engine.nodes_asof import _AsofSide

    S = _AsofSide(device)
    S.words = [tensor_from_portable(w, device) for w in d["words"]]
    S.weights = tensor_from_portable(d["weights"], device)
    S.cols = (
        {n: column_from_portable(c, device) for n, c in d["cols"].items()}
        if d["cols"] is not None
        else None
    )
    return S


def node_state_load(node, state, device) -> None:
    from pathway_amd.engine.nodes_index import VectorIndexState

    kind = state["kind"]
    if kind == "reduce":
        node.seq = state["seq"]
        node.add_keys = (
            [tensor_from_portable(w, device) for w in state["add_keys"]]
            if state["add_keys"] is not None
            else None
        )
        node.add_accs = {
            n: tensor_from_portable(t, device) for n, t in state["add_accs"].items()
        }
        # the low parts (`x__c`) of double-double float sums: created or
        # folded away to suit the node restored into
        node.restore_float_accs()
        node.add_carried = {
            n: column_from_portable(c, device) for n, c in state["add_carried"].items()
        }
        node.multiset_store = _arrangement_from_portable(state["multiset"], device)
    elif kind == "two_store":
        node.lstore = _sidestore_from_portable(state["l"], device)
        node.rstore = _sidestore_from_portable(state["r"], device)
    elif kind == "semi":
        node.lstore = _sidestore_from_portable(state["l"], device)
        node.rcount = _sidestore_from_portable(state["r"], device)
    elif kind == "dedup":
        node.state = state["state"]
    elif kind == "recompute":
        node.stores = [_sidestore_from_portable(s, device) for s in state["stores"]]
        node.prev_output = state["prev"]
    elif kind == "buffer":
        node.watermark = state["wm"]
        node.held = [
            (_batch_from_portable(b, device), tensor_from_portable(t, device))
            for b, t in state["held"]
        ]
    elif kind == "forget":
        node.watermark = state["wm"]
        node.live = [
            (_batch_from_portable(b, device), tensor_from_portable(t, device))
            for b, t in state["live"]
        ]
    elif kind == "freeze":
        node.watermark = state["wm"]
    elif kind == "vindex":
        st = VectorIndexState(device, node.state.metric)
        st.keys = tensor_from_portable(state["keys"], device)
        st.vectors = (
            tensor_from_portable(state["vectors"], device)
            if state["vectors"] is not None
            else None
        )
        st.payload = state["payload"]
        node.state = st
        node.answers = state["answers"]
    elif kind == "bm25":
        node.state = state["state"]
        node.answers = state["answers"]
    elif kind == "asof":
        node.L = _asof_side_from_portable(state["l"], device)
        node.R = _asof_side_from_portable(state["r"], device)
    elif kind == "sorted_side":
        node.S = _asof_side_from_portable(state["s"], device)
