"""BM25 full-text index (reference stdlib/indexing/bm25.py:41 TantivyBM25 +
src/external_integration/tantivy_integration.rs parity).

In-memory inverted index with Okapi BM25 scoring; same as-of-now semantics
and filter support as the KNN retrievers (_BM25IndexNode shares
ExternalIndexNode's protocol).  Two states with one surface:

- _BM25State: host numpy CSR, float64 scores, one query at a time.  Serves
  CPU nodes.
- _BM25DeviceState: tokenisation and the doc log stay on the host; the
  compiled CSR postings live on the node's device, a step's queries are
  scored in one launch of the pw_bm25_score HIP kernel (ops.bm25_score,
  float32) and ranked with pw_topk.  Serves GPU nodes.

PW_BM25=host|device overrides the choice (see internals/config.py).
"""

from __future__ import annotations

import math
import os
import re
from collections import Counter, defaultdict
from dataclasses import dataclass
from typing import Any

import numpy as np
import torch

from pathway_amd.internals import dtype as dt
from pathway_amd.internals import expression as ex
from pathway_amd.internals.api import BasePointer
from pathway_amd.internals.config import get_device


_TOKEN_RE = re.compile(r"[A-Za-z0-9_]+")


def _tokenize(text: str) -> list[str]:
    return [t.lower() for t in _TOKEN_RE.findall(text or "")]


class _BM25State:
    """Okapi BM25 over compiled CSR postings.

    Mutations (add/remove) update the source-of-truth doc maps and mark
    the compiled arrays dirty; the first search after a change rebuilds
    the CSR (vocab ids, per-term [doc_idx, tf] slabs, doc lengths) with
    numpy, and query scoring is fully vectorized (np.add.at scatter +
    argpartition top-k) — the tantivy-scale formulation of the round-1
    dict-loop."""

    def __init__(self, k1: float = 1.2, b: float = 0.75):
        self.k1 = k1
        self.b = b
        self.docs: dict[tuple[int, int], Counter] = {}
        self.doc_len: dict[tuple[int, int], int] = {}
        self.payload: dict[tuple[int, int], Any] = {}
        self._compiled = None  # (keys, doc_len_arr, vocab, offsets, pidx, ptf)

    def add(self, key, text: str, payload=None):
        toks = Counter(_tokenize(text))
        self.docs[key] = toks
        self.doc_len[key] = sum(toks.values())
        if payload is not None:
            self.payload[key] = payload
        self._compiled = None

    def remove(self, key):
        self.docs.pop(key, None)
        self.doc_len.pop(key, None)
        self.payload.pop(key, None)
        self._compiled = None

    def _compile(self):
        if self._compiled is not None:
            return self._compiled
        keys = list(self.docs.keys())
        n = len(keys)
        doc_len_arr = np.array(
            [self.doc_len[k] for k in keys], dtype=np.float64
        )
        vocab: dict[str, int] = {}
        term_ids_per_doc = []
        tfs_per_doc = []
        for k in keys:
            c = self.docs[k]
            tids = np.empty(len(c), dtype=np.int64)
            tfs = np.empty(len(c), dtype=np.int64)
            for j, (t, f) in enumerate(c.items()):
                tid = vocab.get(t)
                if tid is None:
                    tid = vocab[t] = len(vocab)
                tids[j] = tid
                tfs[j] = f
            term_ids_per_doc.append(tids)
            tfs_per_doc.append(tfs)
        if n:
            all_tids = np.concatenate(term_ids_per_doc)
            all_tfs = np.concatenate(tfs_per_doc)
            all_docs = np.repeat(
                np.arange(n, dtype=np.int64),
                [len(a) for a in term_ids_per_doc],
            )
            order = np.argsort(all_tids, kind="stable")
            s_tids = all_tids[order]
            pidx = all_docs[order]
            ptf = all_tfs[order].astype(np.float64)
            counts = np.bincount(s_tids, minlength=len(vocab))
            offsets = np.zeros(len(vocab) + 1, dtype=np.int64)
            np.cumsum(counts, out=offsets[1:])
        else:
            pidx = np.zeros(0, dtype=np.int64)
            ptf = np.zeros(0, dtype=np.float64)
            offsets = np.zeros(1, dtype=np.int64)
        self._compiled = (keys, doc_len_arr, vocab, offsets, pidx, ptf)
        return self._compiled

    def search(self, query: str, k: int, filter_spec=None):
        from pathway_amd.engine.nodes_index import _apply_filter

        n = len(self.docs)
        if n == 0:
            return []
        keys, doc_len_arr, vocab, offsets, pidx, ptf = self._compile()
        avgdl = float(doc_len_arr.mean()) if n else 1.0
        scores = np.zeros(n, dtype=np.float64)
        norm = self.k1 * (1 - self.b + self.b * doc_len_arr / max(avgdl, 1e-9))
        for t in set(_tokenize(query)):
            tid = vocab.get(t)
            if tid is None:
                continue
            s, e = offsets[tid], offsets[tid + 1]
            df = e - s
            idf = math.log(1 + (n - df + 0.5) / (df + 0.5))
            d = pidx[s:e]
            f = ptf[s:e]
            contrib = idf * (f * (self.k1 + 1)) / (f + norm[d])
            np.add.at(scores, d, contrib)
        nz = np.nonzero(scores > 0)[0]
        if nz.size == 0:
            return []
        # rank: top-k among scored docs (argpartition then sort)
        take = min(max(k * 4, k), nz.size) if filter_spec is not None else min(k, nz.size)
        part = nz[np.argpartition(-scores[nz], take - 1)[:take]]
        ranked = part[np.argsort(-scores[part], kind="stable")]
        out = []
        for di in ranked:
            key = keys[di]
            if filter_spec is not None:
                try:
                    if not _apply_filter(filter_spec, self.payload.get(key)):
                        continue
                except Exception:
                    continue
            out.append((key, float(scores[di])))
            if len(out) >= k:
                return out
        if filter_spec is not None and len(out) < k:
            # filtered short: fall back to the full ranked list
            full = nz[np.argsort(-scores[nz], kind="stable")]
            for di in full[take:]:
                key = keys[di]
                try:
                    if not _apply_filter(filter_spec, self.payload.get(key)):
                        continue
                except Exception:
                    continue
                out.append((key, float(scores[di])))
                if len(out) >= k:
                    break
        return out


#: byte budget of the dense (queries, docs) float32 score matrix of one
#: bm25_score launch; search_batch chunks over queries to stay under it
_SCORE_BUDGET_BYTES = 256 * 1024 * 1024

#: largest k that pw_topk selects (PW_TOPK_MAXK)
_TOPK_MAXK = 32

#: pw_topk runs one block per row, so on one long row it is a single block
#: streaming the whole row.  Rows longer than this are ranked in two
#: stages: pw_topk over segments of this many columns, then pw_topk over
#: the segments' candidates.
_TOPK_SEG = 8192


def _topk_rows(scores: torch.Tensor, k: int):
    """Per-row top-k (vals, idx), best first, of a (rows, m) float32 score
    matrix with k <= min(m, _TOPK_MAXK): torch.topk on CPU tensors, pw_topk
    on the GPU, in two stages when m is a multiple of _TOPK_SEG above it.
    Equal scores rank in no defined order."""
    from pathway_amd import ops

    if not scores.is_cuda:
        return torch.topk(scores, k, dim=1)
    nrows, m = scores.shape
    if m <= _TOPK_SEG or m % _TOPK_SEG:
        return ops.topk_gpu(scores, k)
    nseg = m // _TOPK_SEG
    seg_vals, seg_idx = ops.topk_gpu(scores.view(nrows * nseg, _TOPK_SEG), k)
    vals, pos = ops.topk_gpu(seg_vals.view(nrows, nseg * k), k)
    idx = seg_idx.view(nrows, nseg * k).gather(1, pos) + (pos // k) * _TOPK_SEG
    return vals, idx


class _BM25DeviceState:
    """Okapi BM25 with the compiled postings and the scoring on a torch
    device (the GPU in production; the same code runs on CPU tensors).

    Same add / remove / search surface as _BM25State, plus search_batch,
    which answers a whole step's queries with one ops.bm25_score launch
    per chunk of the score budget.

    The source of truth stays on the host, as an append-only slot log: a
    slot per add() holding the key, the doc length, and the doc's
    (term_id, tf) pairs as numpy arrays against a growing vocab.  remove()
    (and a re-add of a live key) only marks the slot dead.  The first
    search after a change compiles: the flat arrays go to the device, dead
    slots are masked out there, one stable sort by term id plus
    bincount/cumsum gives offsets / pidx / ptf with doc slots ascending
    within each term, and norm is computed on the device.  No step of the
    compile loops over documents in Python.  Once more than half of the
    log is dead it is rewritten without the dead slots.

    Scores are float32 (_BM25State's are float64).  Ties rank in no
    defined order, as on the host.  Pickling drops the compiled arrays;
    they are rebuilt on the next search."""

    def __init__(self, k1: float = 1.2, b: float = 0.75, device="cpu"):
        self.k1 = k1
        self.b = b
        self.device = str(device)
        self.vocab: dict[str, int] = {}
        self.payload: dict[tuple[int, int], Any] = {}
        self._slot_of: dict[tuple[int, int], int] = {}
        self._slot_keys: list = []
        self._slot_len: list[int] = []
        self._slot_nterms: list[int] = []
        self._slot_alive = bytearray()
        self._tid_chunks: list[np.ndarray] = []  # int32, one per slot
        self._tf_chunks: list[np.ndarray] = []  # float32, one per slot
        self._compiled = None

    def __len__(self) -> int:
        return len(self._slot_of)

    def __getstate__(self):
        st = dict(self.__dict__)
        st["_compiled"] = None
        return st

    def add(self, key, text: str, payload=None):
        self.remove(key)
        toks = Counter(_tokenize(text))
        vocab = self.vocab
        tids = np.fromiter(
            (vocab.setdefault(t, len(vocab)) for t in toks),
            dtype=np.int32,
            count=len(toks),
        )
        tfs = np.fromiter(toks.values(), dtype=np.float32, count=len(toks))
        self._slot_of[key] = len(self._slot_keys)
        self._slot_keys.append(key)
        self._slot_len.append(sum(toks.values()))
        self._slot_nterms.append(len(toks))
        self._slot_alive.append(1)
        self._tid_chunks.append(tids)
        self._tf_chunks.append(tfs)
        if payload is not None:
            self.payload[key] = payload
        self._compiled = None

    def remove(self, key):
        slot = self._slot_of.pop(key, None)
        if slot is None:
            return
        self._slot_alive[slot] = 0
        self.payload.pop(key, None)
        self._compiled = None

    def _flatten(self):
        """The slot log's postings as two flat arrays (cached in place)."""
        if len(self._tid_chunks) != 1:
            self._tid_chunks = [
                np.concatenate(self._tid_chunks)
                if self._tid_chunks
                else np.zeros(0, dtype=np.int32)
            ]
            self._tf_chunks = [
                np.concatenate(self._tf_chunks)
                if self._tf_chunks
                else np.zeros(0, dtype=np.float32)
            ]
        return self._tid_chunks[0], self._tf_chunks[0]

    def _compact(self, alive: np.ndarray, nterms: np.ndarray):
        """Rewrite the slot log without its dead slots."""
        from itertools import compress

        flat_tid, flat_tf = self._flatten()
        keep = np.repeat(alive, nterms)
        self._tid_chunks = [flat_tid[keep]]
        self._tf_chunks = [flat_tf[keep]]
        self._slot_keys = list(compress(self._slot_keys, self._slot_alive))
        self._slot_len = list(compress(self._slot_len, self._slot_alive))
        self._slot_nterms = nterms[alive].tolist()
        self._slot_alive = bytearray(b"\x01") * len(self._slot_keys)
        self._slot_of = dict(zip(self._slot_keys, range(len(self._slot_keys))))

    def _compile(self):
        """(keys, offsets on device, offsets on host, pidx, ptf, norm) of
        the live docs; doc slot i of the compiled arrays is keys[i]."""
        if self._compiled is not None:
            return self._compiled
        from itertools import compress

        dev = torch.device(self.device)
        alive = np.frombuffer(self._slot_alive, dtype=np.uint8).astype(bool)
        nterms = np.asarray(self._slot_nterms, dtype=np.int64)
        if alive.size and 2 * int(alive.sum()) < alive.size:
            self._compact(alive, nterms)
            alive = np.ones(len(self._slot_keys), dtype=bool)
            nterms = np.asarray(self._slot_nterms, dtype=np.int64)
        flat_tid, flat_tf = self._flatten()
        all_alive = bool(alive.all())
        keys = (
            list(self._slot_keys)
            if all_alive
            else list(compress(self._slot_keys, self._slot_alive))
        )
        n = len(keys)
        V = len(self.vocab)
        assert n < 2**31 and flat_tid.size < 2**31
        tid = torch.from_numpy(flat_tid).to(dev)
        tf = torch.from_numpy(flat_tf).to(dev)
        nterms_d = torch.from_numpy(nterms).to(dev)
        dl = torch.tensor(self._slot_len, dtype=torch.float64, device=dev)
        if all_alive:
            doc_of_slot = torch.arange(n, dtype=torch.int32, device=dev)
        else:
            alive_d = torch.from_numpy(alive).to(dev)
            doc_of_slot = (torch.cumsum(alive_d, 0) - 1).to(torch.int32)
            keep = torch.repeat_interleave(alive_d, nterms_d)
            dl = dl[alive_d]
        pdoc = torch.repeat_interleave(doc_of_slot, nterms_d)
        if not all_alive:
            tid, tf, pdoc = tid[keep], tf[keep], pdoc[keep]
        # stable: doc slots stay ascending within each term
        s_tid, order = torch.sort(tid, stable=True)
        pidx = pdoc[order].contiguous()
        ptf = tf[order].contiguous()
        offsets = torch.zeros(V + 1, dtype=torch.int64, device=dev)
        if s_tid.numel():
            torch.cumsum(
                torch.bincount(s_tid, minlength=V), 0, out=offsets[1:]
            )
        # float64 on the device, rounded once: norm carries one rounding
        avgdl = max(float(dl.sum().item()) / n, 1e-9) if n else 1.0
        norm = (self.k1 * (1 - self.b + self.b * dl / avgdl)).to(torch.float32)
        self._compiled = (keys, offsets, offsets.cpu().numpy(), pidx, ptf, norm)
        return self._compiled

    def _batch_terms(self, queries, wanted=None):
        """The query batch in CSR form: (counts (nq,) int64, term ids int32,
        idf float32).  A query's terms are its distinct known terms that
        have a live posting, ids ascending; a query with wanted[i] false
        gets none.  idf is computed in float64 from the compiled offsets,
        for the whole batch at once, and rounded once."""
        offsets_h = self._compile()[2]
        n = len(self._slot_of)
        vocab = self.vocab
        flat: list[int] = []
        qidx: list[int] = []
        for qi, query in enumerate(queries):
            if wanted is not None and not wanted[qi]:
                continue
            ids = sorted({vocab[t] for t in _tokenize(query) if t in vocab})
            flat += ids
            qidx += [qi] * len(ids)
        tids = np.asarray(flat, dtype=np.int64)
        df = (offsets_h[tids + 1] - offsets_h[tids]).astype(np.float64)
        live = df > 0
        tids, df = tids[live], df[live]
        counts = np.bincount(
            np.asarray(qidx, dtype=np.int64)[live], minlength=len(queries)
        )
        idf = np.log(1 + (n - df + 0.5) / (df + 0.5))
        return counts, tids.astype(np.int32), idf.astype(np.float32)

    def _query_terms(self, query: str):
        """(term ids int32, idf float32) of one query (see _batch_terms)."""
        return self._batch_terms([query])[1:]

    def search(self, query: str, k: int, filter_spec=None):
        return self.search_batch([query], [k], [filter_spec])[0]

    def search_batch(self, queries, ks, filters=None):
        """[(key, score), ...] best-first for every query; ks and filters
        are per query (filters may be None, or hold None entries)."""
        from pathway_amd import ops

        nq = len(queries)
        out: list[list] = [[] for _ in range(nq)]
        n = len(self._slot_of)
        if nq == 0 or n == 0:
            return out
        if filters is None:
            filters = [None] * nq
        ks = [int(k) for k in ks]
        keys, offsets, _, pidx, ptf, norm = self._compile()
        dev = norm.device
        counts, tids, idf = self._batch_terms(queries, [k > 0 for k in ks])
        # a query with no known term stays []: it takes no row of a launch
        active = np.nonzero(counts)[0]
        if active.size == 0:
            return out
        ends = np.cumsum(counts)
        tids_d = torch.from_numpy(tids).to(dev)
        idf_d = torch.from_numpy(idf).to(dev)
        # rows long enough for the two-stage top-k are padded to whole segments
        pad_to = _TOPK_SEG if dev.type == "cuda" and n > _TOPK_SEG else 1
        n_pad = -(-n // pad_to) * pad_to
        chunk = max(1, _SCORE_BUDGET_BYTES // (4 * n_pad))
        for c0 in range(0, active.size, chunk):
            rows = active[c0 : c0 + chunk]
            t0 = ends[rows[0]] - counts[rows[0]]
            t1 = ends[rows[-1]]
            q_off = np.empty(rows.size + 1, dtype=np.int32)
            q_off[0] = 0
            q_off[1:] = ends[rows] - t0
            rows = rows.tolist()
            scores = ops.bm25_score(
                offsets,
                pidx,
                ptf,
                norm,
                torch.from_numpy(q_off).to(dev),
                tids_d[t0:t1],
                idf_d[t0:t1],
                self.k1,
                pad_to,
            )
            fast = [
                r
                for r, qi in enumerate(rows)
                if ks[qi] <= _TOPK_MAXK and filters[qi] is None
            ]
            if fast:
                kmax = min(max(ks[rows[r]] for r in fast), n)
                sub = scores if len(fast) == len(rows) else scores[
                    torch.tensor(fast, device=dev)
                ]
                vals, idx = _topk_rows(sub, kmax)
                vals, idx = vals.tolist(), idx.tolist()
                for j, r in enumerate(fast):
                    qi = rows[r]
                    out[qi] = [
                        (keys[d], s)
                        for s, d in zip(vals[j][: ks[qi]], idx[j][: ks[qi]])
                        if s > 0
                    ]
            fast_set = set(fast)
            for r, qi in enumerate(rows):
                if r not in fast_set:
                    out[qi] = self._select_row(
                        scores[r, :n], keys, ks[qi], filters[qi]
                    )
        return out

    def _select_row(self, row: torch.Tensor, keys, k: int, filter_spec):
        """The host's selection on one dense score row: top max(4k, k)
        candidates when filtering (k otherwise), filter on the host, and
        the rest of the ranked row if that yields fewer than k."""
        from pathway_amd.engine.nodes_index import _apply_filter

        def passes(key):
            if filter_spec is None:
                return True
            try:
                return bool(_apply_filter(filter_spec, self.payload.get(key)))
            except Exception:
                return False

        n = row.shape[0]
        take = min(max(k * 4, k), n) if filter_spec is not None else min(k, n)
        vals, idx = torch.topk(row, take)
        out = []
        for s, d in zip(vals.tolist(), idx.tolist()):
            if s <= 0:
                return out  # sorted: nothing scored is left
            if passes(keys[d]):
                out.append((keys[d], s))
                if len(out) >= k:
                    return out
        if filter_spec is not None and take < n:
            # filtered short: fall back to the full ranked row
            vals, idx = torch.sort(row, descending=True, stable=True)
            for s, d in zip(vals[take:].tolist(), idx[take:].tolist()):
                if s <= 0:
                    break
                if passes(keys[d]):
                    out.append((keys[d], s))
                    if len(out) >= k:
                        break
        return out


def _use_device_state(device) -> bool:
    """The device state serves GPU nodes; PW_BM25=host|device overrides."""
    mode = os.environ.get("PW_BM25", "").strip().lower()
    if mode not in ("", "host", "device"):
        raise ValueError(f"PW_BM25 must be 'host' or 'device', got {mode!r}")
    if mode:
        return mode == "device"
    return torch.device(device).type == "cuda"


class TantivyBM25:
    """InnerIndex retriever over the text column (reference bm25.py:41)."""

    def __init__(
        self,
        data_column: ex.ColumnReference,
        metadata_column: ex.ColumnReference | None = None,
        *,
        ram_budget: int = 50_000_000,
        in_memory_index: bool = True,
        k1: float = 1.2,
        b: float = 0.75,
    ):
        self.data_column = data_column
        self.metadata_column = metadata_column
        self.k1 = k1
        self.b = b
        self.embedder = None  # API parity with KNN retrievers

    def query_as_of_now(self, query_column, number_of_matches: int = 3, metadata_filter=None):
        from pathway_amd.engine.nodes_index import ExternalIndexNode
        from pathway_amd.internals.table import Table

        data_table = self.data_column.table
        query_table = query_column.table
        index_src = data_table
        text_name = self.data_column.name
        filter_col = None
        if self.metadata_column is not None:
            index_src = index_src.with_columns(_pw_meta=self.metadata_column)
            filter_col = "_pw_meta"
        node = _BM25IndexNode(
            index_src._node,
            query_table._node,
            text_name,
            query_column,
            number_of_matches,
            get_device(),
            filter_data_col=filter_col,
            query_filter_expr=metadata_filter,
            k1=self.k1,
            b=self.b,
        )
        dtypes = {
            "_pw_index_reply_ids": dt.List(dt.POINTER),
            "_pw_index_reply_scores": dt.List(dt.FLOAT),
        }
        return Table(node, dtypes, query_table._universe)

    query = query_as_of_now


@dataclass
class TantivyBM25Factory:
    ram_budget: int = 50_000_000
    in_memory_index: bool = True

    def build_index(self, data_column, metadata_column=None, **kwargs) -> TantivyBM25:
        return TantivyBM25(data_column, metadata_column)


from pathway_amd.engine.nodes import Node as _Node


class _BM25IndexNode(_Node):
    """Engine node sharing ExternalIndexNode's protocol, BM25 scoring."""

    def __init__(
        self,
        index_node,
        query_node,
        text_col: str,
        query_expr,
        k: int,
        device,
        filter_data_col=None,
        query_filter_expr=None,
        k1: float = 1.2,
        b: float = 0.75,
    ):
        super().__init__([index_node, query_node], device)
        self.text_col = text_col
        self.query_expr = query_expr
        self.k = int(k) if not isinstance(k, ex.ColumnExpression) else 16
        self.k_expr = k if isinstance(k, ex.ColumnExpression) else None
        self.filter_data_col = filter_data_col
        self.query_filter_expr = query_filter_expr
        self.state = self._new_state(k1, b)
        self.answers: dict = {}

    def _new_state(self, k1, b):
        if _use_device_state(self.device):
            return _BM25DeviceState(k1, b, self.device)
        return _BM25State(k1, b)

    def reset(self):
        self.state = self._new_state(self.state.k1, self.state.b)
        self.answers = {}

    def step(self, time, inputs):
        from pathway_amd.engine.batch import DeltaBatch
        from pathway_amd.engine.column import obj_array, ObjectColumn
        from pathway_amd.engine.expression_eval import EvalContext, evaluate

        bi, bq = inputs
        if bi is not None and len(bi):
            texts = bi.columns[self.text_col].to_pylist()
            payloads = (
                bi.columns[self.filter_data_col].to_pylist()
                if self.filter_data_col and self.filter_data_col in bi.columns
                else [None] * len(bi)
            )
            diffs = bi.diffs.cpu().tolist()
            keys = bi.keys.cpu().tolist()
            for i in range(len(bi)):
                key = tuple(keys[i])
                if diffs[i] > 0:
                    self.state.add(key, texts[i], payloads[i])
                else:
                    self.state.remove(key)
        if bq is None or len(bq) == 0:
            return None
        ctx = EvalContext(bq.columns, bq.keys, self.device)
        queries = evaluate(self.query_expr, ctx).to_pylist()
        ks = None
        if self.k_expr is not None:
            ks = [int(v) for v in evaluate(self.k_expr, ctx).to_pylist()]
        filts = None
        if self.query_filter_expr is not None:
            filts = evaluate(self.query_filter_expr, ctx).to_pylist()
        qkeys = bq.keys.cpu().tolist()
        diffs = bq.diffs.cpu().tolist()
        # every positive-diff row of the step is answered against the same
        # index state: one batched search where the state has one
        pos = [i for i in range(len(bq)) if diffs[i] > 0]
        pos_q = [queries[i] or "" for i in pos]
        pos_k = [ks[i] if ks else self.k for i in pos]
        pos_f = [filts[i] if filts else None for i in pos]
        if hasattr(self.state, "search_batch"):
            pos_hits = self.state.search_batch(pos_q, pos_k, pos_f)
        else:
            pos_hits = [
                self.state.search(q, k, f) for q, k, f in zip(pos_q, pos_k, pos_f)
            ]
        hits_of = dict(zip(pos, pos_hits))
        out_rows = []
        for i in range(len(bq)):
            key = tuple(qkeys[i])
            if diffs[i] > 0:
                hits = hits_of[i]
                ids = tuple(
                    BasePointer.from_signed_pair(h[0][0], h[0][1]) for h in hits
                )
                scores = tuple(float(h[1]) for h in hits)
                vals = (ids, scores)
                self.answers[key] = vals
                out_rows.append((qkeys[i], vals, diffs[i]))
            else:
                vals = self.answers.pop(key, ((), ()))
                out_rows.append((qkeys[i], vals, diffs[i]))
        keys_t = torch.tensor(
            [r[0] for r in out_rows], dtype=torch.int64, device=self.device
        ).reshape(len(out_rows), 2)
        diffs_t = torch.tensor(
            [r[2] for r in out_rows], dtype=torch.int64, device=self.device
        )
        return DeltaBatch(
            keys_t,
            {
                "_pw_index_reply_ids": ObjectColumn(
                    obj_array([r[1][0] for r in out_rows]), dt.List(dt.POINTER)
                ),
                "_pw_index_reply_scores": ObjectColumn(
                    obj_array([r[1][1] for r in out_rows]), dt.List(dt.FLOAT)
                ),
            },
            diffs_t,
            time,
        )
