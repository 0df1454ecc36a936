"""pathway_amd.ops — native HIP/CDNA4 kernel bindings (ctypes, no shims).

On a GPU host the hash hot path MUST run through libpwhip.so; if the
library is missing there we raise instead of silently falling back to the
torch reference implementation (which only serves as the CPU path and the
numerics reference for the kernels).
"""

from __future__ import annotations

import contextlib
import ctypes
import os
from typing import Sequence

import torch

_THIS = os.path.dirname(os.path.abspath(__file__))
_LIB_PATH = os.path.join(_THIS, "libpwhip.so")

_lib = None
_load_error: Exception | None = None


def _try_load():
    global _lib, _load_error
    if _lib is not None:
        return _lib
    try:
        if not os.path.exists(_LIB_PATH):
            from pathway_amd.ops import build as _build

            _build.build(verbose=False)
        _lib = ctypes.CDLL(_LIB_PATH)
        _lib.pw_hash128_words.restype = ctypes.c_int
        _lib.pw_value_hash.restype = ctypes.c_int
        _lib.pw_varlen_hash.restype = ctypes.c_int
        _lib.pw_run_starts.restype = ctypes.c_int
    except Exception as e:  # noqa: BLE001
        _load_error = e
        _lib = None
    return _lib


def lib_available() -> bool:
    return _try_load() is not None


def require_lib():
    lib = _try_load()
    if lib is None:
        raise RuntimeError(
            f"pathway_amd native HIP library missing on a GPU host: {_load_error}"
        )
    return lib


def _stream_ptr() -> ctypes.c_void_p:
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


#: widest row k_hash128_words is instantiated for
HASH_MAX_WORDS = 20


def hash128_words_gpu(words: Sequence[torch.Tensor]) -> tuple[torch.Tensor, torch.Tensor]:
    """Fused device 128-bit hash of rows of int64 words: 1 to HASH_MAX_WORDS
    1-D int64 tensors of one length on one device."""
    lib = require_lib()
    if not 1 <= len(words) <= HASH_MAX_WORDS:
        raise ValueError(
            f"hash128_words_gpu takes 1..{HASH_MAX_WORDS} words, got {len(words)}"
        )
    n = words[0].shape[0]
    for w in words:
        if w.dtype != torch.int64:
            raise ValueError(f"hash128_words_gpu needs int64 words, got {w.dtype}")
        if w.dim() != 1 or w.shape[0] != n:
            raise ValueError("hash128_words_gpu needs 1-D words of one length")
        if w.device != words[0].device:
            raise ValueError("hash128_words_gpu needs all words on one device")
    lo = torch.empty(n, dtype=torch.int64, device=words[0].device)
    hi = torch.empty(n, dtype=torch.int64, device=words[0].device)
    # the contiguous copies stay referenced until the launch is queued
    words = [w.contiguous() for w in words]
    arr = (ctypes.c_void_p * len(words))(
        *[ctypes.c_void_p(w.data_ptr()) for w in words]
    )
    rc = lib.pw_hash128_words(
        arr,
        ctypes.c_int(len(words)),
        ctypes.c_int64(n),
        ctypes.c_void_p(lo.data_ptr()),
        ctypes.c_void_p(hi.data_ptr()),
        _stream_ptr(),
    )
    if rc != 0:
        raise RuntimeError(f"pw_hash128_words failed: hip error {rc}")
    return lo, hi


def value_hash_gpu(payload: torch.Tensor, tag: int) -> tuple[torch.Tensor, torch.Tensor]:
    lib = require_lib()
    payload = payload.contiguous()
    n = payload.shape[0]
    lo = torch.empty(n, dtype=torch.int64, device=payload.device)
    hi = torch.empty(n, dtype=torch.int64, device=payload.device)
    rc = lib.pw_value_hash(
        ctypes.c_void_p(payload.data_ptr()),
        ctypes.c_uint64(tag),
        ctypes.c_int64(n),
        ctypes.c_void_p(lo.data_ptr()),
        ctypes.c_void_p(hi.data_ptr()),
        _stream_ptr(),
    )
    if rc != 0:
        raise RuntimeError(f"pw_value_hash failed: hip error {rc}")
    return lo, hi


def varlen_hash_gpu(
    bytes_t: torch.Tensor, offsets: torch.Tensor, tag: int
) -> tuple[torch.Tensor, torch.Tensor]:
    """Device hash of varlen byte rows: offsets (n+1,) int64, bytes uint8."""
    lib = require_lib()
    n = offsets.shape[0] - 1
    lo = torch.empty(n, dtype=torch.int64, device=bytes_t.device)
    hi = torch.empty(n, dtype=torch.int64, device=bytes_t.device)
    bytes_t = bytes_t.contiguous()
    rc = lib.pw_varlen_hash(
        ctypes.c_void_p(bytes_t.data_ptr()),
        ctypes.c_int64(bytes_t.numel()),
        ctypes.c_void_p(offsets.contiguous().data_ptr()),
        ctypes.c_uint64(tag),
        ctypes.c_int64(n),
        ctypes.c_void_p(lo.data_ptr()),
        ctypes.c_void_p(hi.data_ptr()),
        _stream_ptr(),
    )
    if rc != 0:
        raise RuntimeError(f"pw_varlen_hash failed: hip error {rc}")
    return lo, hi


def run_starts_gpu(words: Sequence[torch.Tensor]) -> torch.Tensor:
    lib = require_lib()
    n = words[0].shape[0]
    starts = torch.empty(n, dtype=torch.bool, device=words[0].device)
    arr = (ctypes.c_void_p * len(words))(
        *[ctypes.c_void_p(w.contiguous().data_ptr()) for w in words]
    )
    rc = lib.pw_run_starts(
        arr,
        ctypes.c_int(len(words)),
        ctypes.c_int64(n),
        ctypes.c_void_p(starts.data_ptr()),
        _stream_ptr(),
    )
    if rc != 0:
        raise RuntimeError(f"pw_run_starts failed: hip error {rc}")
    return starts


def host_hash128_bytes(data: bytes) -> tuple[int, int]:
    lib = require_lib()
    lo = ctypes.c_uint64()
    hi = ctypes.c_uint64()
    lib.pw_host_hash128_bytes(data, ctypes.c_int64(len(data)), ctypes.byref(lo), ctypes.byref(hi))
    return lo.value, hi.value


def _ptr_arr(tensors):
    return (ctypes.c_void_p * len(tensors))(
        *[ctypes.c_void_p(t.data_ptr()) for t in tensors]
    )


def searchsorted_gpu(
    sorted_words: Sequence[torch.Tensor],
    query_words: Sequence[torch.Tensor],
    side: str = "left",
) -> torch.Tensor:
    lib = require_lib()
    m = sorted_words[0].shape[0]
    nq = query_words[0].shape[0]
    out = torch.empty(nq, dtype=torch.int64, device=query_words[0].device)
    s = [t.contiguous() for t in sorted_words]
    q = [t.contiguous() for t in query_words]
    rc = lib.pw_searchsorted(
        _ptr_arr(s),
        _ptr_arr(q),
        ctypes.c_int(len(s)),
        ctypes.c_int64(m),
        ctypes.c_int64(nq),
        ctypes.c_int(1 if side == "right" else 0),
        ctypes.c_void_p(out.data_ptr()),
        _stream_ptr(),
    )
    if rc != 0:
        raise RuntimeError(f"pw_searchsorted failed: hip error {rc}")
    return out


def lookup_gpu(
    sorted_words: Sequence[torch.Tensor], query_words: Sequence[torch.Tensor]
) -> tuple[torch.Tensor, torch.Tensor]:
    lib = require_lib()
    m = sorted_words[0].shape[0]
    nq = query_words[0].shape[0]
    pos = torch.empty(nq, dtype=torch.int64, device=query_words[0].device)
    found = torch.empty(nq, dtype=torch.bool, device=query_words[0].device)
    s = [t.contiguous() for t in sorted_words]
    q = [t.contiguous() for t in query_words]
    rc = lib.pw_lookup(
        _ptr_arr(s),
        _ptr_arr(q),
        ctypes.c_int(len(s)),
        ctypes.c_int64(m),
        ctypes.c_int64(nq),
        ctypes.c_void_p(pos.data_ptr()),
        ctypes.c_void_p(found.data_ptr()),
        _stream_ptr(),
    )
    if rc != 0:
        raise RuntimeError(f"pw_lookup failed: hip error {rc}")
    return pos, found


def key_range_gpu(
    sorted_words: Sequence[torch.Tensor], query_words: Sequence[torch.Tensor]
) -> tuple[torch.Tensor, torch.Tensor]:
    lib = require_lib()
    m = sorted_words[0].shape[0]
    nq = query_words[0].shape[0]
    lo = torch.empty(nq, dtype=torch.int64, device=query_words[0].device)
    hi = torch.empty(nq, dtype=torch.int64, device=query_words[0].device)
    s = [t.contiguous() for t in sorted_words]
    q = [t.contiguous() for t in query_words]
    rc = lib.pw_key_range(
        _ptr_arr(s),
        _ptr_arr(q),
        ctypes.c_int(len(s)),
        ctypes.c_int64(m),
        ctypes.c_int64(nq),
        ctypes.c_void_p(lo.data_ptr()),
        ctypes.c_void_p(hi.data_ptr()),
        _stream_ptr(),
    )
    if rc != 0:
        raise RuntimeError(f"pw_key_range failed: hip error {rc}")
    return lo, hi


#: modes of seg_select_gpu
SEG_FIRST = 0
SEG_MIN = 1
SEG_MAX = 2
#: seg_select_gpu: a range of more rows than this is finished by the second
#: launch, one 1024-thread workgroup per range (profiles/multiset_r09.md)
SEG_SELECT_LONG = 4096
#: seg_distinct_gpu: entries of the per-range LDS table; one pass fills
#: GC_BUCKET_MAX_LOAD of it at the most and a range takes at most 64 passes
SEG_DISTINCT_CAPACITY = 4096
SEG_DISTINCT_MAX_PASSES = 64

#: which path served each GroupReduceNode._multiset_agg call: the segmented
#: select kernel, the segmented distinct kernel, the per-group host loop, or
#: the torch scatter chain of min/max
multiset_path_counts = {"select": 0, "distinct": 0, "host": 0, "torch": 0}


def _check_ranges(lo: torch.Tensor, hi: torch.Tensor, weights: torch.Tensor):
    for name, t in (("lo", lo), ("hi", hi), ("weights", weights)):
        if t.dtype != torch.int64 or t.dim() != 1 or not t.is_contiguous():
            raise ValueError(f"{name} must be a contiguous 1-D int64 tensor")
        if not t.is_cuda or t.device != weights.device:
            raise ValueError(f"{name} must be on the weights' GPU")
    if lo.shape[0] != hi.shape[0]:
        raise ValueError("lo and hi differ in length")


def seg_select_gpu(
    lo: torch.Tensor,
    hi: torch.Tensor,
    weights: torch.Tensor,
    key: torch.Tensor | None,
    mode: int,
    long_rows: int | None = None,
) -> torch.Tensor:
    """The chosen store row of every range [lo[q], hi[q]), or -1 where the
    range holds no row of positive weight (pw_seg_select; no host read).

    Rows with weights[r] <= 0 are skipped in every mode.  SEG_FIRST takes
    the smallest row index that is left and reads no key.  SEG_MIN / SEG_MAX
    take the smallest / largest key; equal keys go to the smallest row
    index.  int64 keys compare as int64.  float64 keys compare with < and >,
    so -0.0 and 0.0 tie; a NaN key beats every number in both modes, and
    NaNs tie by row index.  Ranges of more than `long_rows` rows (default
    SEG_SELECT_LONG) are finished by a second launch."""
    lib = require_lib()
    _check_ranges(lo, hi, weights)
    m = weights.shape[0]
    if mode == SEG_FIRST:
        if key is not None:
            raise ValueError("SEG_FIRST reads no key")
        kind, kptr = 0, None
    elif mode in (SEG_MIN, SEG_MAX):
        if key is None:
            raise ValueError("SEG_MIN / SEG_MAX need a key column")
        if key.dtype == torch.int64:
            kind = 1
        elif key.dtype == torch.float64:
            kind = 2
        else:
            raise ValueError(f"key must be int64 or float64, not {key.dtype}")
        if key.shape != (m,) or not key.is_contiguous() or key.device != weights.device:
            raise ValueError("key must be a contiguous 1-D column of the store")
        kptr = key.data_ptr()
    else:
        raise ValueError(f"unknown mode {mode}")
    long_rows = SEG_SELECT_LONG if long_rows is None else int(long_rows)
    if long_rows < 64:
        raise ValueError("long_rows must be at least 64")
    nq = lo.shape[0]
    sel = torch.empty(nq, dtype=torch.int64, device=weights.device)
    rc = lib.pw_seg_select(
        ctypes.c_void_p(lo.data_ptr()),
        ctypes.c_void_p(hi.data_ptr()),
        ctypes.c_int64(nq),
        ctypes.c_void_p(weights.data_ptr()),
        ctypes.c_void_p(kptr),
        ctypes.c_int(kind),
        ctypes.c_int64(m),
        ctypes.c_int(mode),
        ctypes.c_int64(long_rows),
        ctypes.c_void_p(sel.data_ptr()),
        _stream_ptr(),
    )
    if rc != 0:
        raise RuntimeError(f"pw_seg_select failed: error {rc}")
    return sel


def seg_distinct_gpu(
    lo: torch.Tensor,
    hi: torch.Tensor,
    weights: torch.Tensor,
    values: torch.Tensor,
    table_capacity: int | None = None,
) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(count, first, status) of every range [lo[q], hi[q]): the number of
    distinct int64 `values` among its rows of positive weight, the first
    such row (-1 if none), and status 0 = exact, 1 = given up with count 0
    (pw_seg_distinct; no host read).

    One workgroup per range with a set of `table_capacity` entries (default
    SEG_DISTINCT_CAPACITY) in LDS.  A range of more distinct values than
    GC_BUCKET_MAX_LOAD of the table is counted in a power-of-two number of
    passes over disjoint hash classes, found by doubling; one that needs
    more than SEG_DISTINCT_MAX_PASSES (any range of more than
    SEG_DISTINCT_MAX_PASSES * GC_BUCKET_MAX_LOAD * table_capacity distinct
    values does), or an insert that runs past GC_BUCKET_MAX_PROBE slots,
    gives the range up, with first -1.  Every int64 is a value, -1
    included."""
    lib = require_lib()
    _check_ranges(lo, hi, weights)
    m = weights.shape[0]
    if (
        values.dtype != torch.int64
        or values.shape != (m,)
        or not values.is_contiguous()
        or values.device != weights.device
    ):
        raise ValueError("values must be a contiguous 1-D int64 column of the store")
    cap = SEG_DISTINCT_CAPACITY if table_capacity is None else int(table_capacity)
    if cap < 64 or cap > 8192 or cap & (cap - 1):
        raise ValueError("table_capacity must be a power of two in [64, 8192]")
    nq = lo.shape[0]
    dev = weights.device
    count = torch.empty(nq, dtype=torch.int64, device=dev)
    first = torch.empty(nq, dtype=torch.int64, device=dev)
    status = torch.empty(nq, dtype=torch.int32, device=dev)
    rc = lib.pw_seg_distinct(
        ctypes.c_void_p(lo.data_ptr()),
        ctypes.c_void_p(hi.data_ptr()),
        ctypes.c_int64(nq),
        ctypes.c_void_p(weights.data_ptr()),
        ctypes.c_void_p(values.data_ptr()),
        ctypes.c_int64(m),
        ctypes.c_int64(cap),
        ctypes.c_int64(int(GC_BUCKET_MAX_LOAD * cap)),
        ctypes.c_int64(GC_BUCKET_MAX_PROBE),
        ctypes.c_void_p(count.data_ptr()),
        ctypes.c_void_p(first.data_ptr()),
        ctypes.c_void_p(status.data_ptr()),
        _stream_ptr(),
    )
    if rc != 0:
        raise RuntimeError(f"pw_seg_distinct failed: error {rc}")
    return count, first, status


def pool_hash_gpu(
    codes: torch.Tensor,
    pool_lo: torch.Tensor,
    pool_hi: torch.Tensor,
    none_lo: int,
    none_hi: int,
) -> tuple[torch.Tensor, torch.Tensor]:
    lib = require_lib()
    n = codes.shape[0]
    lo = torch.empty(n, dtype=torch.int64, device=codes.device)
    hi = torch.empty(n, dtype=torch.int64, device=codes.device)
    rc = lib.pw_pool_hash(
        ctypes.c_void_p(codes.contiguous().data_ptr()),
        ctypes.c_void_p(pool_lo.contiguous().data_ptr()),
        ctypes.c_void_p(pool_hi.contiguous().data_ptr()),
        ctypes.c_uint64(none_lo & ((1 << 64) - 1)),
        ctypes.c_uint64(none_hi & ((1 << 64) - 1)),
        ctypes.c_int64(n),
        ctypes.c_void_p(lo.data_ptr()),
        ctypes.c_void_p(hi.data_ptr()),
        _stream_ptr(),
    )
    if rc != 0:
        raise RuntimeError(f"pw_pool_hash failed: hip error {rc}")
    return lo, hi


def varlen_hash_se_gpu(
    bytes_t: torch.Tensor,
    starts: torch.Tensor,
    ends: torch.Tensor,
    tag: int,
) -> tuple[torch.Tensor, torch.Tensor]:
    """Device hash of varlen rows with explicit [start, end) spans."""
    lib = require_lib()
    n = starts.shape[0]
    lo = torch.empty(n, dtype=torch.int64, device=bytes_t.device)
    hi = torch.empty(n, dtype=torch.int64, device=bytes_t.device)
    bytes_t = bytes_t.contiguous()
    rc = lib.pw_varlen_hash_se(
        ctypes.c_void_p(bytes_t.data_ptr()),
        ctypes.c_int64(bytes_t.numel()),
        ctypes.c_void_p(starts.contiguous().data_ptr()),
        ctypes.c_void_p(ends.contiguous().data_ptr()),
        ctypes.c_uint64(tag),
        ctypes.c_int64(n),
        ctypes.c_void_p(lo.data_ptr()),
        ctypes.c_void_p(hi.data_ptr()),
        _stream_ptr(),
    )
    if rc != 0:
        raise RuntimeError(f"pw_varlen_hash_se failed: hip error {rc}")
    return lo, hi


def hash_agg_gpu(
    k0: torch.Tensor,
    k1: torch.Tensor,
    contribs: Sequence[torch.Tensor],
    expected_uniques: int | None = None,
) -> tuple[torch.Tensor, torch.Tensor, list, torch.Tensor] | None:
    """Sort-free additive pre-aggregation (pw_hash_agg): returns
    (uk0, uk1, [accs...], rep_row_idx) for the distinct group keys of the
    batch — UNSORTED and possibly with rare duplicate keys (publication
    race); callers sort + consolidate the (small) result.

    expected_uniques sizes the table at ~2x that (L2-resident when the
    estimate is vocabulary-scale — the round-1 A/B lost because the 2n
    table was a 270 MB HBM random walk).  Returns None if the estimate
    was too small (probe-chain overflow): redo on the sort path with a
    bigger estimate.

    Limits: at most 8 accumulators; k0 == INT64_MIN is the table's empty
    mark and must not occur; and since the table's second words start at
    0, a row with k1 == 0 can be added to a slot that another key with
    the same k0 has claimed but not yet published.  Keys are 128-bit
    hashes, so neither happens in practice."""
    lib = require_lib()
    n = k0.shape[0]
    dev = k0.device
    nacc = len(contribs)
    est = n if expected_uniques is None else min(max(expected_uniques, 512), n)
    cap = 1 << max(10, (2 * est - 1).bit_length())
    out_cap = min(n, cap)
    tk0 = torch.empty(cap, dtype=torch.int64, device=dev)
    tk1 = torch.zeros(cap, dtype=torch.int64, device=dev)
    rep = torch.zeros(cap, dtype=torch.int64, device=dev)
    taccs = [torch.zeros(cap, dtype=torch.int64, device=dev) for _ in range(nacc)]
    counter = torch.zeros(2, dtype=torch.int32, device=dev)  # [count, overflow]
    out_k0 = torch.empty(out_cap, dtype=torch.int64, device=dev)
    out_k1 = torch.empty(out_cap, dtype=torch.int64, device=dev)
    out_rep = torch.empty(out_cap, dtype=torch.int64, device=dev)
    out_accs = [
        torch.empty(out_cap, dtype=torch.int64, device=dev) for _ in range(nacc)
    ]
    carr = (ctypes.c_void_p * max(nacc, 1))(
        *[ctypes.c_void_p(c.contiguous().data_ptr()) for c in contribs]
    )
    tarr = (ctypes.c_void_p * max(nacc, 1))(
        *[ctypes.c_void_p(c.data_ptr()) for c in taccs]
    )
    oarr = (ctypes.c_void_p * max(nacc, 1))(
        *[ctypes.c_void_p(c.data_ptr()) for c in out_accs]
    )
    rc = lib.pw_hash_agg(
        ctypes.c_void_p(k0.contiguous().data_ptr()),
        ctypes.c_void_p(k1.contiguous().data_ptr()),
        carr,
        ctypes.c_int(nacc),
        ctypes.c_int64(n),
        ctypes.c_void_p(tk0.data_ptr()),
        ctypes.c_void_p(tk1.data_ptr()),
        tarr,
        ctypes.c_void_p(rep.data_ptr()),
        ctypes.c_int64(cap),
        ctypes.c_void_p(counter.data_ptr()),
        ctypes.c_void_p(out_k0.data_ptr()),
        ctypes.c_void_p(out_k1.data_ptr()),
        oarr,
        ctypes.c_void_p(out_rep.data_ptr()),
        ctypes.c_void_p(counter.data_ptr() + 4),
        _stream_ptr(),
    )
    if rc != 0:
        raise RuntimeError(f"pw_hash_agg failed: hip error {rc}")
    # counter is the only host-visible size: one small D2H sync
    m, overflowed = (int(x) for x in counter.tolist())
    if overflowed:
        return None
    return (
        out_k0.narrow(0, 0, m),
        out_k1.narrow(0, 0, m),
        [a.narrow(0, 0, m) for a in out_accs],
        out_rep.narrow(0, 0, m),
    )


def seg_reduce_words_gpu(
    words: Sequence[torch.Tensor], contribs: Sequence[torch.Tensor]
) -> tuple[list, torch.Tensor, list]:
    """Fused segmented reduce over rows SORTED by `words` (≤8 int64 word
    columns): returns (unique word columns, first_row_idx, [per-seg int64
    sums...]) — the whole run-starts/compaction/segment-sum chain in two
    kernels + one tiny cumsum.  At most 8 accumulators; sums wrap modulo
    2^64.  No rows in, no rows out."""
    lib = require_lib()
    n = words[0].shape[0]
    dev = words[0].device
    nw = len(words)
    nacc = len(contribs)
    if nw > 8 or nacc > 8:
        raise RuntimeError(
            f"seg_reduce_words_gpu: {nw} words, {nacc} accumulators (8 at the most)"
        )
    if n == 0:
        empty = lambda: torch.empty(0, dtype=torch.int64, device=dev)  # noqa: E731
        return [empty() for _ in range(nw)], empty(), [empty() for _ in range(nacc)]
    words = [w.contiguous() for w in words]
    nblocks = (n + 255) // 256
    block_counts = torch.empty(nblocks, dtype=torch.int32, device=dev)
    warr = (ctypes.c_void_p * nw)(
        *[ctypes.c_void_p(w.data_ptr()) for w in words]
    )
    rc = lib.pw_seg_reduce_count(
        warr,
        ctypes.c_int(nw),
        ctypes.c_int64(n),
        ctypes.c_void_p(block_counts.data_ptr()),
        ctypes.c_int64(nblocks),
        _stream_ptr(),
    )
    if rc != 0:
        raise RuntimeError(f"pw_seg_reduce_count failed: hip error {rc}")
    csum = torch.cumsum(block_counts.to(torch.int64), 0)
    nseg = int(csum[-1].item())
    bases = torch.cat(
        [torch.zeros(1, dtype=torch.int64, device=dev), csum[:-1]]
    )
    out_words = [torch.empty(nseg, dtype=torch.int64, device=dev) for _ in range(nw)]
    out_first = torch.empty(nseg, dtype=torch.int64, device=dev)
    out_accs = [torch.zeros(nseg, dtype=torch.int64, device=dev) for _ in range(nacc)]
    carr = (ctypes.c_void_p * max(nacc, 1))(
        *[ctypes.c_void_p(c.contiguous().data_ptr()) for c in contribs]
    )
    oarr = (ctypes.c_void_p * max(nacc, 1))(
        *[ctypes.c_void_p(c.data_ptr()) for c in out_accs]
    )
    owarr = (ctypes.c_void_p * nw)(
        *[ctypes.c_void_p(w.data_ptr()) for w in out_words]
    )
    rc = lib.pw_seg_reduce_emit(
        warr,
        ctypes.c_int(nw),
        carr,
        ctypes.c_int(nacc),
        ctypes.c_int64(n),
        ctypes.c_void_p(bases.data_ptr()),
        owarr,
        ctypes.c_void_p(out_first.data_ptr()),
        oarr,
        ctypes.c_int64(nblocks),
        _stream_ptr(),
    )
    if rc != 0:
        raise RuntimeError(f"pw_seg_reduce_emit failed: hip error {rc}")
    return out_words, out_first, out_accs


def seg_reduce_gpu(
    k0: torch.Tensor, k1: torch.Tensor, contribs: Sequence[torch.Tensor]
) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor, list]:
    """2-word convenience wrapper over seg_reduce_words_gpu."""
    out_words, out_first, out_accs = seg_reduce_words_gpu([k0, k1], contribs)
    return out_words[0], out_words[1], out_first, out_accs


#: rocPRIM temp-storage bytes of the group-combine sorts, per row count
_gc_temp_bytes: dict[int, int] = {}
_gc_temp_bytes_prefix: dict[int, int] = {}

#: PW_GC_FULL_SORT=1 forces the 64-bit sort of word0 (A/B runs)
_PW_GC_FULL_SORT = bool(os.environ.get("PW_GC_FULL_SORT"))

#: which path group_combine_gpu ran: the prefix sort, the 64-bit sort after
#: the prefix path overflowed, the 64-bit sort because it was asked for, or
#: the bucket path (one radix pass + per-bucket LDS aggregation) where the
#: caller enabled it and it held
class _GcPathCounts(dict):
    """The three sort counts as plain dict entries, as their tests snapshot
    and compare them, plus the "bucket" count, read and written by key but
    left out of iteration and copies."""

    bucket = 0

    def __getitem__(self, key):
        return self.bucket if key == "bucket" else dict.__getitem__(self, key)

    def __setitem__(self, key, value):
        if key == "bucket":
            self.bucket = value
        else:
            dict.__setitem__(self, key, value)


gc_path_counts = _GcPathCounts({"prefix": 0, "fallback": 0, "full": 0})

#: PW_NO_GC_PARTITION=1 keeps the bucket path on its sort-and-gather layout
_PW_NO_GC_PARTITION = bool(os.environ.get("PW_NO_GC_PARTITION"))
#: PW_GC_PART_DIRECT=1 scatters the partition from registers instead of
#: ordering it in LDS first (A/B runs, profiles/wordcount_r10.md)
_PW_GC_PART_DIRECT = bool(os.environ.get("PW_GC_PART_DIRECT"))
#: how a bucket-path call that held laid its rows out: moved into bucket
#: order by the partition kernels, or sorted by bucket and gathered
gc_bucket_layout_counts = {"partition": 0, "gather": 0}
#: rows per workgroup of the partition kernels (PW_GC_PT_TILE)
GC_PART_TILE = 8192
#: the partition layout serves at most this many bucket bits
GC_PART_MAX_BITS = 8

#: whether a group_combine_gpu call that does not say `bucket=` tries the
#: bucket path; the groupby node sets it around its call (gc_bucket_scope)
_gc_bucket_scope = False


@contextlib.contextmanager
def gc_bucket_scope(on: bool):
    """Within the block, group_combine_gpu calls without a `bucket`
    argument try the bucket path iff `on`."""
    global _gc_bucket_scope
    old, _gc_bucket_scope = _gc_bucket_scope, bool(on)
    try:
        yield
    finally:
        _gc_bucket_scope = old

#: prefix runs the last prefix-path call listed for repair
gc_last_dirty_runs = 0

#: bucket path: share of a bucket's LDS table that distinct keys may fill
GC_BUCKET_MAX_LOAD = 0.5
#: bucket path defaults (profiles/wordcount_r07.md): one onesweep radix pass
GC_BUCKET_BITS = 8
#: bucket path: a bucket may hold this many times its even share of the rows
GC_BUCKET_ROWS_FACTOR = 4
#: bucket path: slots one insert may probe; far beyond any chain of a table
#: at GC_BUCKET_MAX_LOAD, and it bounds the work once a table has filled up
GC_BUCKET_MAX_PROBE = 128
GC_BUCKET_ROWS_FLOOR = 65536

_gc_bucket_caps: dict[int, int] = {}


def gc_bucket_capacity_limit(nacc: int) -> int:
    """Largest power-of-two `table_capacity` whose table, with `nacc` sums
    per entry, fits the aggregation kernel's LDS (60 KB, so that two
    workgroups share a CU)."""
    cap = _gc_bucket_caps.get(nacc)
    if cap is None:
        fn = require_lib().pw_gc_bucket_max_capacity
        fn.restype = ctypes.c_int64
        cap = int(fn(ctypes.c_int(nacc)))
        if cap < 2:
            raise RuntimeError("pw_gc_bucket_max_capacity failed")
        _gc_bucket_caps[nacc] = cap
    return cap


def gc_bucket_capacity(nacc: int) -> int:
    """Default `table_capacity` of the bucket path: the limit, at most 2048."""
    return min(gc_bucket_capacity_limit(nacc), 2048)


def gc_bucket_key_budget(nacc: int, bucket_bits: int = GC_BUCKET_BITS,
                         table_capacity: int | None = None) -> int:
    """Distinct keys the bucket path holds when they spread evenly."""
    cap = table_capacity or gc_bucket_capacity(nacc)
    return (1 << bucket_bits) * int(GC_BUCKET_MAX_LOAD * cap)


def _gc_temp(lib, n: int, prefix: bool, dev) -> tuple[torch.Tensor, int]:
    cache = _gc_temp_bytes_prefix if prefix else _gc_temp_bytes
    tbytes = cache.get(n)
    if tbytes is None:
        fn = lib.pw_gc_temp_bytes_prefix if prefix else lib.pw_gc_temp_bytes
        fn.restype = ctypes.c_int64
        tbytes = int(fn(ctypes.c_int64(n)))
        if tbytes <= 0:
            raise RuntimeError("pw_gc_temp_bytes failed")
        cache[n] = tbytes
    return torch.empty(tbytes, dtype=torch.uint8, device=dev), tbytes


def _gc_two_sorts(keys_n2, contribs):
    """The combiners' last resort, for a batch in which more rows than
    the repair's `max_run` share one word0 and differ in word1: two stable
    sorts (word1, then word0), sorted copies of the contributions and
    seg_reduce_gpu.  Same result as the other paths, at several times
    the cost.  After the result: the int64 permutation and every segment's
    start position in it."""
    k0, k1 = keys_n2[:, 0], keys_n2[:, 1]
    perm = torch.argsort(k1, stable=True)
    perm = perm.index_select(0, torch.argsort(k0.index_select(0, perm), stable=True))
    uk0, uk1, first_sorted, accs = seg_reduce_gpu(
        k0.index_select(0, perm),
        k1.index_select(0, perm),
        [c.index_select(0, perm) for c in contribs],
    )
    first_row = perm.index_select(0, first_sorted)
    return uk0, uk1, first_row, accs, perm, first_sorted


def _gc_part_hist_entries(lib, n: int, bucket_bits: int) -> int:
    fn = lib.pw_gc_part_hist_entries
    fn.restype = ctypes.c_int64
    entries = int(fn(ctypes.c_int64(n), ctypes.c_int(bucket_bits)))
    if entries <= 0:
        raise RuntimeError("pw_gc_part_hist_entries failed")
    tile = lib.pw_gc_part_tile
    tile.restype = ctypes.c_int64
    assert int(tile()) == GC_PART_TILE
    return entries


def _gc_aligned_keys(keys_n2: torch.Tensor) -> torch.Tensor:
    """The partition kernels read a key as one 128-bit load."""
    return keys_n2.clone() if keys_n2.data_ptr() % 16 else keys_n2


def gc_partition_gpu(
    keys_n2: torch.Tensor, contribs: Sequence[torch.Tensor], bucket_bits: int
) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor, list]:
    """The partition step of the bucket path on its own, for tests
    (k_gc_part_count, _scan, _scatter): (bucket_start (2^bits + 1) int64,
    part_keys (n,2), part_row (n) int64, part_accs), the rows grouped by
    bucket in signed key order, in no particular order inside a bucket."""
    lib = require_lib()
    n = keys_n2.shape[0]
    dev = keys_n2.device
    nacc = len(contribs)
    assert keys_n2.dim() == 2 and keys_n2.shape[1] == 2
    assert keys_n2.dtype == torch.int64
    assert 2 <= n < 2**32 - 1 and nacc <= 8 and 1 <= bucket_bits <= 8
    if keys_n2.stride() != (2, 1):
        keys_n2 = keys_n2.contiguous()
    keys_n2 = _gc_aligned_keys(keys_n2)
    contribs = [c.contiguous() for c in contribs]
    assert all(c.dtype == torch.int64 and c.shape == (n,) for c in contribs)
    nb = 1 << bucket_bits
    hist = _gc_part_hist_entries(lib, n, bucket_bits)
    part64 = torch.empty((2 + nacc, n), dtype=torch.int64, device=dev)
    # block_hist, part_row, bucket_start (uint32 bits)
    scratch32 = torch.empty(hist + n + nb + 1, dtype=torch.int32, device=dev)
    ctl = torch.empty(2, dtype=torch.int64, device=dev)
    carr = (ctypes.c_void_p * max(nacc, 1))(
        *[ctypes.c_void_p(c.data_ptr()) for c in contribs]
    )
    parr = (ctypes.c_void_p * max(nacc, 1))(
        *[ctypes.c_void_p(part64[2 + a].data_ptr()) for a in range(nacc)]
    )
    rc = lib.pw_gc_partition(
        ctypes.c_void_p(keys_n2.data_ptr()),
        ctypes.c_int64(n),
        ctypes.c_int(bucket_bits),
        carr,
        ctypes.c_int(nacc),
        ctypes.c_void_p(scratch32.data_ptr()),
        ctypes.c_void_p(part64.data_ptr()),
        ctypes.c_void_p(scratch32[hist:].data_ptr()),
        parr,
        ctypes.c_void_p(scratch32[hist + n :].data_ptr()),
        ctypes.c_void_p(ctl.data_ptr()),
        ctypes.c_int(int(_PW_GC_PART_DIRECT)),
        _stream_ptr(),
    )
    if rc != 0:
        raise RuntimeError(f"pw_gc_partition failed: hip error {rc}")
    u32 = lambda t: t.to(torch.int64) & 0xFFFFFFFF  # noqa: E731
    return (
        u32(scratch32[hist + n :]),
        part64[:2].reshape(n, 2),
        u32(scratch32[hist : hist + n]),
        [part64[2 + a] for a in range(nacc)],
    )


def _group_combine_bucket(
    lib, keys_n2, contribs, bucket_bits, table_capacity, max_bucket_rows,
    partition=False,
):
    """group_combine_gpu's bucket path (pw_gc_bucket_*).  Returns the
    result, or None when a bucket overflowed its table, its row limit or
    the probe bound.  One host read: total unique keys + overflow word.
    `partition`: the rows are moved into bucket order (pw_gc_bucket_part_agg,
    bucket_bits <= 8) instead of being sorted by bucket and gathered."""
    n = keys_n2.shape[0]
    dev = keys_n2.device
    nacc = len(contribs)
    nb = 1 << bucket_bits
    max_distinct = max(1, int(GC_BUCKET_MAX_LOAD * table_capacity))
    stream = _stream_ptr()
    # bucket_start (nb+1), bucket_uniques (nb)
    bounds = torch.empty(2 * nb + 1, dtype=torch.int32, device=dev)
    # base (nb+1), then total and overflow word for one read
    base_ctl = torch.empty(nb + 3, dtype=torch.int64, device=dev)
    carr = (ctypes.c_void_p * max(nacc, 1))(
        *[ctypes.c_void_p(c.data_ptr()) for c in contribs]
    )
    if partition:
        keys_n2 = _gc_aligned_keys(keys_n2)
        hist = _gc_part_hist_entries(lib, n, bucket_bits)
        # block_hist, part_row, st_first (uint32 bits)
        scratch32 = torch.empty(hist + 2 * n, dtype=torch.int32, device=dev)
        st_first = scratch32[hist + n :]
        # part_keys (n,2), nacc partitioned columns, then the staging rows
        staged = torch.empty(
            (2 + nacc + 2 + max(nacc, 1), n), dtype=torch.int64, device=dev
        )
        st0 = 2 + nacc
        parr = (ctypes.c_void_p * max(nacc, 1))(
            *[ctypes.c_void_p(staged[2 + a].data_ptr()) for a in range(nacc)]
        )
    else:
        temp, tbytes = _gc_temp(lib, n, True, dev)
        scratch32 = torch.empty((3, n), dtype=torch.int32, device=dev)  # uint32 bits
        st_first = scratch32[2]
        staged = torch.empty((2 + max(nacc, 1), n), dtype=torch.int64, device=dev)
        st0 = 0
    sarr = (ctypes.c_void_p * max(nacc, 1))(
        *[ctypes.c_void_p(staged[st0 + 2 + a].data_ptr()) for a in range(nacc)]
    )
    if partition:
        rc = lib.pw_gc_bucket_part_agg(
            ctypes.c_void_p(keys_n2.data_ptr()),
            ctypes.c_int64(n),
            ctypes.c_int(bucket_bits),
            ctypes.c_int64(table_capacity),
            ctypes.c_int64(max_distinct),
            ctypes.c_int64(max_bucket_rows),
            ctypes.c_int64(min(table_capacity, GC_BUCKET_MAX_PROBE)),
            carr,
            ctypes.c_int(nacc),
            ctypes.c_void_p(scratch32.data_ptr()),
            ctypes.c_void_p(staged.data_ptr()),
            ctypes.c_void_p(scratch32[hist:].data_ptr()),
            parr,
            ctypes.c_void_p(bounds.data_ptr()),
            ctypes.c_void_p(bounds[nb + 1 :].data_ptr()),
            ctypes.c_void_p(base_ctl.data_ptr()),
            ctypes.c_void_p(staged[st0].data_ptr()),
            ctypes.c_void_p(staged[st0 + 1].data_ptr()),
            ctypes.c_void_p(st_first.data_ptr()),
            sarr,
            ctypes.c_void_p(base_ctl[nb + 1 :].data_ptr()),
            ctypes.c_int(int(_PW_GC_PART_DIRECT)),
            stream,
        )
    else:
        rc = lib.pw_gc_bucket_agg(
            ctypes.c_void_p(keys_n2.data_ptr()),
            ctypes.c_int64(n),
            ctypes.c_void_p(temp.data_ptr()),
            ctypes.c_int64(tbytes),
            ctypes.c_void_p(scratch32[0].data_ptr()),
            ctypes.c_void_p(scratch32[1].data_ptr()),
            ctypes.c_int(bucket_bits),
            ctypes.c_int64(table_capacity),
            ctypes.c_int64(max_distinct),
            ctypes.c_int64(max_bucket_rows),
            ctypes.c_int64(min(table_capacity, GC_BUCKET_MAX_PROBE)),
            carr,
            ctypes.c_int(nacc),
            ctypes.c_void_p(bounds.data_ptr()),
            ctypes.c_void_p(bounds[nb + 1 :].data_ptr()),
            ctypes.c_void_p(base_ctl.data_ptr()),
            ctypes.c_void_p(staged[0].data_ptr()),
            ctypes.c_void_p(staged[1].data_ptr()),
            ctypes.c_void_p(st_first.data_ptr()),
            sarr,
            ctypes.c_void_p(base_ctl[nb + 1 :].data_ptr()),
            stream,
        )
    if rc != 0:
        fn = "pw_gc_bucket_part_agg" if partition else "pw_gc_bucket_agg"
        raise RuntimeError(f"{fn} failed: hip error {rc}")
    total, overflow = base_ctl[nb + 1 :].tolist()
    if overflow:
        return None
    out_k = torch.empty((2, total), dtype=torch.int64, device=dev)
    out_first = torch.empty(total, dtype=torch.int64, device=dev)
    out_accs = torch.empty((max(nacc, 1), total), dtype=torch.int64, device=dev)
    oarr = (ctypes.c_void_p * max(nacc, 1))(
        *[ctypes.c_void_p(out_accs[a].data_ptr()) for a in range(nacc)]
    )
    rc = lib.pw_gc_bucket_compact(
        ctypes.c_void_p(base_ctl.data_ptr()),
        ctypes.c_void_p(bounds.data_ptr()),
        ctypes.c_int(bucket_bits),
        ctypes.c_int64(total),
        ctypes.c_void_p(staged[st0].data_ptr()),
        ctypes.c_void_p(staged[st0 + 1].data_ptr()),
        ctypes.c_void_p(st_first.data_ptr()),
        sarr,
        ctypes.c_int(nacc),
        ctypes.c_void_p(out_k[0].data_ptr()),
        ctypes.c_void_p(out_k[1].data_ptr()),
        ctypes.c_void_p(out_first.data_ptr()),
        oarr,
        stream,
    )
    if rc != 0:
        raise RuntimeError(f"pw_gc_bucket_compact failed: hip error {rc}")
    return out_k[0], out_k[1], out_first, [out_accs[a] for a in range(nacc)]


def _gc_sort_count(lib, keys_n2, prefix_bits, max_run, max_dirty, full_sort):
    """The sort half of group_combine_gpu and group_combine_mixed_gpu: the
    prefix path (sort, gather, repair, count), on overflow or `full_sort`
    the 64-bit sort.  Returns (sorted_k (2,n), perm32, block csum, nseg),
    or None when the 64-bit sort's repair overflowed too."""
    global gc_last_dirty_runs
    n = keys_n2.shape[0]
    dev = keys_n2.device
    sorted_k = torch.empty((2, n), dtype=torch.int64, device=dev)
    perm32 = torch.empty(n, dtype=torch.int32, device=dev)  # uint32 bits
    nblocks = (n + 255) // 256
    block_counts = torch.empty(nblocks, dtype=torch.int32, device=dev)
    # block csum, then the prefix path's two control words (overflow,
    # listed runs), so that one read fetches nseg and the overflow word
    csum_ctrl = torch.empty(nblocks + 2, dtype=torch.int64, device=dev)
    csum = csum_ctrl[:nblocks]
    dirty_list = torch.empty(max_dirty, dtype=torch.int32, device=dev)
    stream = _stream_ptr()
    full_sort = full_sort or _PW_GC_FULL_SORT
    nseg = -1
    if not full_sort:
        temp, tbytes = _gc_temp(lib, n, True, dev)
        rc = lib.pw_gc_prefix_sort_count(
            ctypes.c_void_p(keys_n2.data_ptr()),
            ctypes.c_int64(n),
            ctypes.c_void_p(temp.data_ptr()),
            ctypes.c_int64(tbytes),
            ctypes.c_void_p(sorted_k[0].data_ptr()),
            ctypes.c_void_p(sorted_k[1].data_ptr()),
            ctypes.c_void_p(perm32.data_ptr()),
            ctypes.c_int(prefix_bits),
            ctypes.c_int64(max_run),
            ctypes.c_int64(max_dirty),
            ctypes.c_void_p(dirty_list.data_ptr()),
            ctypes.c_void_p(csum_ctrl[nblocks:].data_ptr()),
            ctypes.c_void_p(block_counts.data_ptr()),
            stream,
        )
        if rc != 0:
            raise RuntimeError(f"pw_gc_prefix_sort_count failed: hip error {rc}")
        torch.cumsum(block_counts, 0, dtype=torch.int64, out=csum)
        nseg, overflow, gc_last_dirty_runs = csum_ctrl[nblocks - 1 :].tolist()
        if overflow:
            nseg = -1
        else:
            gc_path_counts["prefix"] += 1
    if nseg < 0:
        temp, tbytes = _gc_temp(lib, n, False, dev)
        rc = lib.pw_gc_sort_count(
            ctypes.c_void_p(keys_n2.data_ptr()),
            ctypes.c_int64(n),
            ctypes.c_void_p(temp.data_ptr()),
            ctypes.c_int64(tbytes),
            ctypes.c_void_p(sorted_k[0].data_ptr()),
            ctypes.c_void_p(sorted_k[1].data_ptr()),
            ctypes.c_void_p(perm32.data_ptr()),
            ctypes.c_int(4),
            ctypes.c_int64(max_run),
            ctypes.c_int64(max_dirty),
            ctypes.c_void_p(dirty_list.data_ptr()),
            ctypes.c_void_p(csum_ctrl[nblocks:].data_ptr()),
            ctypes.c_void_p(block_counts.data_ptr()),
            stream,
        )
        if rc != 0:
            raise RuntimeError(f"pw_gc_sort_count failed: hip error {rc}")
        torch.cumsum(block_counts, 0, dtype=torch.int64, out=csum)
        nseg, overflow, _ = csum_ctrl[nblocks - 1 :].tolist()
        gc_path_counts["full" if full_sort else "fallback"] += 1
        if overflow:
            return None
    return sorted_k, perm32, csum, nseg


def _gc_emit(lib, sorted_k, perm32, csum, nseg, contribs, seg_pos=None):
    """The emit half: (uk0, uk1, first_row, accs) from the sorted keys,
    the int64 contributions read through the permutation.  `seg_pos`
    (nseg + 1 int64) also receives every segment's start position in
    sorted order and the row count (pw_gc_emit_pos)."""
    n = perm32.shape[0]
    dev = perm32.device
    nacc = len(contribs)
    out_k = torch.empty((2, nseg), dtype=torch.int64, device=dev)
    out_first = torch.empty(nseg, dtype=torch.int64, device=dev)
    out_accs = torch.zeros((max(nacc, 1), nseg), dtype=torch.int64, device=dev)
    carr = (ctypes.c_void_p * max(nacc, 1))(
        *[ctypes.c_void_p(c.data_ptr()) for c in contribs]
    )
    oarr = (ctypes.c_void_p * max(nacc, 1))(
        *[ctypes.c_void_p(out_accs[a].data_ptr()) for a in range(nacc)]
    )
    args = [
        ctypes.c_void_p(sorted_k[0].data_ptr()),
        ctypes.c_void_p(sorted_k[1].data_ptr()),
        ctypes.c_void_p(perm32.data_ptr()),
        carr,
        ctypes.c_int(nacc),
        ctypes.c_int64(n),
        ctypes.c_void_p(csum.data_ptr()),
        ctypes.c_void_p(out_k[0].data_ptr()),
        ctypes.c_void_p(out_k[1].data_ptr()),
        ctypes.c_void_p(out_first.data_ptr()),
        oarr,
    ]
    if seg_pos is None:
        rc = lib.pw_gc_emit(*args, _stream_ptr())
    else:
        assert seg_pos.shape == (nseg + 1,) and seg_pos.dtype == torch.int64
        rc = lib.pw_gc_emit_pos(
            *args, ctypes.c_void_p(seg_pos.data_ptr()), _stream_ptr()
        )
    if rc != 0:
        raise RuntimeError(f"pw_gc_emit failed: hip error {rc}")
    return out_k[0], out_k[1], out_first, [out_accs[a] for a in range(nacc)]


def group_combine_gpu(
    keys_n2: torch.Tensor,
    contribs: Sequence[torch.Tensor],
    *,
    prefix_bits: int = 32,
    max_run: int = 2048,
    max_dirty: int = 65536,
    full_sort: bool = False,
    bucket: bool | None = None,
    bucket_bits: int = GC_BUCKET_BITS,
    table_capacity: int | None = None,
    max_bucket_rows: int | None = None,
    partition: bool | None = None,
) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor, list]:
    """The groupby combiner on UNSORTED interleaved keys: (n,2) int64 keys
    + up to 8 int64 contribution columns -> (uk0, uk1, first_row, accs)
    with unique keys in signed lexicographic order, per-key sums and the
    smallest input row of every key (pw_gc_*: rocPRIM sort of the top
    `prefix_bits` of word0 with a 32-bit row-index payload read straight
    from the interleaved rows, one gather of both words, an exact repair of
    the rows that tie on the prefix, then a segmented reduce that reads the
    contributions through the permutation).  One host sync (segment count
    and the repair's overflow word in one read).

    A prefix run longer than `max_run` rows, or more than `max_dirty` runs
    to repair, overflows: the batch is redone with the 64-bit sort of word0
    (a second sync).  `full_sort` (or PW_GC_FULL_SORT=1) takes the 64-bit
    sort at once.  That path repairs ties on the whole of word0 under the
    same two caps; beyond them it hands over to two full sorts.  The
    result is the same on every path.

    `bucket=True` (off by default; the groupby node turns it on, through
    gc_bucket_scope, when its estimate of the distinct keys fits) first tries the bucket path: the
    rows are grouped by the top `bucket_bits` of word0, then one workgroup
    per bucket aggregates its rows in an LDS table of `table_capacity`
    entries (a power of two, default gc_bucket_capacity(nacc)) and emits
    its unique keys in order.  It needs no order of the n rows and has one
    host sync too.  With `bucket_bits` <= 8 the grouping is a hand-written
    partition (count, scan, scatter) that moves key, row index and
    contributions into bucket order, so the aggregation reads them in
    sequence; `partition=False` (or PW_NO_GC_PARTITION=1), and any larger
    `bucket_bits`, sorts (prefix, row) pairs by bucket instead and gathers
    the rows through the permutation.  `gc_bucket_layout_counts` says which.  A bucket with more than GC_BUCKET_MAX_LOAD * table_capacity
    distinct keys or more than `max_bucket_rows` rows (default: four times
    the even share, at least 65536) overflows, and the call goes on with
    the prefix path as if `bucket` had not been given."""
    lib = require_lib()
    n = keys_n2.shape[0]
    nacc = len(contribs)
    assert keys_n2.dim() == 2 and keys_n2.shape[1] == 2
    assert keys_n2.dtype == torch.int64
    assert 2 <= n < 2**32 and nacc <= 8
    assert 1 <= prefix_bits <= 32 and 2 <= max_run <= 3072
    assert 1 <= max_dirty < 2**32
    if keys_n2.stride() != (2, 1):
        keys_n2 = keys_n2.contiguous()
    contribs = [c.contiguous() for c in contribs]
    assert all(c.dtype == torch.int64 and c.shape == (n,) for c in contribs)
    if bucket is None:
        bucket = _gc_bucket_scope
    if bucket and not (full_sort or _PW_GC_FULL_SORT) and n < 2**32 - 1:
        assert 1 <= bucket_bits <= 16
        cap = table_capacity or gc_bucket_capacity(nacc)
        assert 2 <= cap <= gc_bucket_capacity_limit(nacc) and cap & (cap - 1) == 0
        if max_bucket_rows is None:
            even = -(-n // (1 << bucket_bits))
            max_bucket_rows = max(GC_BUCKET_ROWS_FACTOR * even, GC_BUCKET_ROWS_FLOOR)
        assert max_bucket_rows >= 1
        if partition is None:
            partition = not _PW_NO_GC_PARTITION
        partition = bool(partition) and bucket_bits <= GC_PART_MAX_BITS
        res = _group_combine_bucket(
            lib, keys_n2, contribs, bucket_bits, cap, max_bucket_rows, partition
        )
        if res is not None:
            gc_path_counts["bucket"] += 1
            gc_bucket_layout_counts["partition" if partition else "gather"] += 1
            return res
    sorted_ = _gc_sort_count(
        lib, keys_n2, prefix_bits, max_run, max_dirty, full_sort
    )
    if sorted_ is None:
        # thousands of rows share a whole word0 and differ in word1
        return _gc_two_sorts(keys_n2, contribs)[:4]
    return _gc_emit(lib, *sorted_, contribs)


#: rows per chunk of a long segment in pw_seg_sum_f64, and the longest
#: segment one wave reduces on its own (profiles/float_reduce_r12.md)
SEG_SUM_F64_CHUNK = 4096

#: how the groupby node reduced a batch with float64 contributions: the
#: mixed combiner, or the torch sort / index_add_ chain (more than 8
#: accumulators)
f64_combine_counts = {"native": 0, "chain": 0}
#: how group_combine_mixed_gpu ordered the rows: one of gc_path_counts'
#: sorts (which one, that dict says), or the two stable sorts after those
gc_mixed_path_counts = {"sorted": 0, "two_sorts": 0}


def seg_sum_f64_gpu(
    perm: torch.Tensor | None,
    seg_start: torch.Tensor,
    hi_cols: Sequence[torch.Tensor],
    lo_cols: Sequence[torch.Tensor] | None = None,
) -> tuple[list, list]:
    """Segmented double-double sums (pw_seg_sum_f64): for every segment
    `[seg_start[s], seg_start[s+1])` of the positions of `perm`, and each of
    1..8 float64 columns read through `perm`, the sum as a normalised
    (hi, lo) pair.  `perm`: int32 holding uint32 bits, int64, or None for
    the identity; its entries lie in [0, n).  `seg_start`: (nseg+1,) int64
    on the device, ascending from 0 to n.  `lo_cols`: the low parts when
    the inputs are double-doubles themselves.  A segment's result depends
    only on its values in permuted order and its length; there are no
    float atomics and no host read.  A sum whose high part is not finite
    is that high part with lo = 0."""
    lib = require_lib()
    ncol = len(hi_cols)
    assert 1 <= ncol <= 8
    n = hi_cols[0].shape[0]
    dev = hi_cols[0].device
    hi_cols = [c.contiguous() for c in hi_cols]
    assert all(c.dtype == torch.float64 and c.shape == (n,) for c in hi_cols)
    if lo_cols is not None:
        lo_cols = [c.contiguous() for c in lo_cols]
        assert len(lo_cols) == ncol
        assert all(c.dtype == torch.float64 and c.shape == (n,) for c in lo_cols)
    assert seg_start.dtype == torch.int64 and seg_start.dim() == 1
    assert seg_start.shape[0] >= 1 and seg_start.device == dev
    seg_start = seg_start.contiguous()
    nseg = seg_start.shape[0] - 1
    if perm is None:
        mode = 0
    else:
        assert perm.shape == (n,) and perm.device == dev
        assert perm.dtype in (torch.int32, torch.int64)
        perm = perm.contiguous()
        mode = 1 if perm.dtype == torch.int32 else 2
    T = SEG_SUM_F64_CHUNK
    out = torch.empty((2 * ncol, nseg), dtype=torch.float64, device=dev)
    out_hi = [out[2 * c] for c in range(ncol)]
    out_lo = [out[2 * c + 1] for c in range(ncol)]
    if nseg == 0:
        return out_hi, out_lo
    max_list = n // T + 1
    max_slots = n // T + max_list
    # ctl (2, zeroed), list (3 * max_list), desc (2 * max_slots)
    work = torch.empty(2 + 3 * max_list + 2 * max_slots, dtype=torch.int64, device=dev)
    work[:2].zero_()
    parts = torch.empty((2 * ncol, max_slots), dtype=torch.float64, device=dev)
    ptrs = lambda ts: (ctypes.c_void_p * ncol)(  # noqa: E731
        *[ctypes.c_void_p(t.data_ptr()) for t in ts]
    )
    rc = lib.pw_seg_sum_f64(
        ctypes.c_void_p(perm.data_ptr() if mode else 0),
        ctypes.c_int(mode),
        ctypes.c_void_p(seg_start.data_ptr()),
        ctypes.c_int64(nseg),
        ctypes.c_int64(n),
        ptrs(hi_cols),
        ptrs(lo_cols) if lo_cols is not None else None,
        ctypes.c_int(ncol),
        ctypes.c_int64(T),
        ptrs(out_hi),
        ptrs(out_lo),
        ctypes.c_void_p(work.data_ptr()),
        ctypes.c_void_p(work[2:].data_ptr()),
        ctypes.c_void_p(work[2 + 3 * max_list :].data_ptr()),
        ctypes.c_void_p(parts.data_ptr()),
        ctypes.c_int64(max_list),
        ctypes.c_int64(max_slots),
        _stream_ptr(),
    )
    if rc != 0:
        raise RuntimeError(f"pw_seg_sum_f64 failed: error {rc}")
    return out_hi, out_lo


def group_combine_mixed_gpu(
    keys_n2: torch.Tensor,
    contribs: Sequence[torch.Tensor],
    f64_contribs: Sequence[torch.Tensor],
    *,
    prefix_bits: int = 32,
    max_run: int = 2048,
    max_dirty: int = 65536,
    full_sort: bool = False,
) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor, list, list, list]:
    """group_combine_gpu for a batch that also carries float64 columns:
    (uk0, uk1, first_row, accs, f_hi, f_lo), the first four as
    group_combine_gpu returns them for the int64 `contribs`, f_hi / f_lo
    the per-key double-double sums of `f64_contribs` (seg_sum_f64_gpu over
    the same permutation).  The sort paths are group_combine_gpu's, the
    bucket path left out: every one of them keeps equal keys in ascending
    row order, so f_hi and f_lo are the same bits on each.  One host read
    on the prefix path (the segment count)."""
    lib = require_lib()
    n = keys_n2.shape[0]
    nacc = len(contribs)
    nf = len(f64_contribs)
    assert keys_n2.dim() == 2 and keys_n2.shape[1] == 2
    assert keys_n2.dtype == torch.int64
    assert 2 <= n < 2**32 and nf >= 1 and nacc + nf <= 8
    assert 1 <= prefix_bits <= 32 and 2 <= max_run <= 3072
    assert 1 <= max_dirty < 2**32
    if keys_n2.stride() != (2, 1):
        keys_n2 = keys_n2.contiguous()
    contribs = [c.contiguous() for c in contribs]
    assert all(c.dtype == torch.int64 and c.shape == (n,) for c in contribs)
    f64_contribs = [c.contiguous() for c in f64_contribs]
    assert all(c.dtype == torch.float64 and c.shape == (n,) for c in f64_contribs)
    sorted_ = _gc_sort_count(
        lib, keys_n2, prefix_bits, max_run, max_dirty, full_sort
    )
    if sorted_ is None:
        # the two stable sorts, with their int64 permutation
        uk0, uk1, first_row, accs, perm, first_sorted = _gc_two_sorts(
            keys_n2, contribs
        )
        seg_pos = torch.cat([first_sorted, first_sorted.new_full((1,), n)])
        gc_mixed_path_counts["two_sorts"] += 1
    else:
        perm = sorted_[1]
        seg_pos = torch.empty(sorted_[3] + 1, dtype=torch.int64, device=perm.device)
        uk0, uk1, first_row, accs = _gc_emit(lib, *sorted_, contribs, seg_pos)
        gc_mixed_path_counts["sorted"] += 1
    f_hi, f_lo = seg_sum_f64_gpu(perm, seg_pos, f64_contribs)
    return uk0, uk1, first_row, accs, f_hi, f_lo


#: column descriptor kinds of pw_row_ident / pw_consolidate_rows
RI_INT64_TAGGED = 0
RI_POOL_CODE = 1
RI_POINTER = 2
RI_PRECOMPUTED = 3
#: widest batch the fused consolidation takes (20 hash words, as
#: hash128_words_gpu)
RI_MAX_COLS = 10

#: which way consolidate_batch went for a device batch of more than 2048
#: rows: the fused native call, that call redone after its prefix repair
#: overflowed (counted in both), or the hash / sort / gather chain
consolidate_path_counts = {"fused": 0, "overflow": 0, "chain": 0}


def _ri_args(col_descs, n: int, dev):
    """ctypes arrays for a list of column descriptors, and the tensors
    they point into (to be kept alive until the launch is queued).

    A descriptor is a tuple led by its kind:
      (RI_INT64_TAGGED, payload int64 (n,), tag, mask bool (n,) or None)
      (RI_POOL_CODE, codes int64 (n,), pool_lo, pool_hi)
      (RI_POINTER, pairs int64 (n,2), tag)
      (RI_PRECOMPUTED, lo int64 (n,), hi int64 (n,))"""
    nc = len(col_descs)
    assert nc <= RI_MAX_COLS
    m = max(nc, 1)
    kinds = (ctypes.c_int * m)()
    pa = (ctypes.c_void_p * m)()
    pb = (ctypes.c_void_p * m)()
    pc = (ctypes.c_void_p * m)()
    px = (ctypes.c_uint64 * m)()
    keep = []

    def dev_t(t, dtype, shape):
        t = t.to(dev).contiguous()
        assert t.dtype == dtype and tuple(t.shape) == shape, (t.dtype, t.shape)
        keep.append(t)
        return t.data_ptr()

    for j, d in enumerate(col_descs):
        kind = d[0]
        kinds[j] = kind
        if kind == RI_INT64_TAGGED:
            pa[j] = dev_t(d[1], torch.int64, (n,))
            px[j] = d[2] & (2**64 - 1)
            if d[3] is not None:
                pb[j] = dev_t(d[3], torch.bool, (n,))
        elif kind == RI_POOL_CODE:
            pa[j] = dev_t(d[1], torch.int64, (n,))
            assert d[2].dtype == torch.int64 and d[2].shape == d[3].shape
            pb[j] = dev_t(d[2], torch.int64, tuple(d[2].shape))
            pc[j] = dev_t(d[3], torch.int64, tuple(d[3].shape))
        elif kind == RI_POINTER:
            pa[j] = dev_t(d[1], torch.int64, (n, 2))
            px[j] = d[2] & (2**64 - 1)
        elif kind == RI_PRECOMPUTED:
            pa[j] = dev_t(d[1], torch.int64, (n,))
            pb[j] = dev_t(d[2], torch.int64, (n,))
        else:
            raise ValueError(f"unknown row-ident column kind {kind}")
    return (kinds, pa, pb, pc, px, ctypes.c_int(nc)), keep


_none_hash_u64: tuple[int, int] | None = None


def _none_hash():
    global _none_hash_u64
    if _none_hash_u64 is None:
        from pathway_amd.internals.api import hash128, serialize_value

        _none_hash_u64 = tuple(hash128(serialize_value(None)))
    return _none_hash_u64


def row_ident_gpu(keys: torch.Tensor, col_descs) -> torch.Tensor:
    """(n,2) int64 row identities (c0, c1) of a batch, interleaved, in one
    pass (pw_row_ident): bit-identical to the columns' value hashes,
    combine_value_hashes and hash128_words([k0, k1, v0, v1]) in turn."""
    lib = require_lib()
    n = keys.shape[0]
    assert keys.dtype == torch.int64 and keys.dim() == 2 and keys.shape[1] == 2
    assert 1 <= n < 2**32
    keys = keys.contiguous()
    args, keep = _ri_args(col_descs, n, keys.device)
    nlo, nhi = _none_hash()
    ckeys = torch.empty((n, 2), dtype=torch.int64, device=keys.device)
    lib.pw_row_ident.restype = ctypes.c_int
    rc = lib.pw_row_ident(
        ctypes.c_void_p(keys.data_ptr()),
        ctypes.c_int64(n),
        *args,
        ctypes.c_uint64(nlo),
        ctypes.c_uint64(nhi),
        ctypes.c_void_p(ckeys.data_ptr()),
        _stream_ptr(),
    )
    if rc != 0:
        raise RuntimeError(f"pw_row_ident failed: hip error {rc}")
    del keep
    return ckeys


def consolidate_rows_gpu(
    keys: torch.Tensor,
    col_descs,
    diffs: torch.Tensor,
    *,
    prefix_bits: int = 32,
    max_run: int = 2048,
    max_dirty: int = 65536,
    gather_keys: bool = False,
) -> tuple:
    """Consolidation of a device batch in one native call
    (pw_consolidate_rows): (n,2) int64 keys, column descriptors (_ri_args)
    and int64 diffs -> (rows, wsum), or with `gather_keys`
    (rows, wsum, keys.index_select(0, rows)), the keys written by the
    kernel that compacts the rows.

    Ordering contract: the rows are grouped by their 128-bit identity
    (c0, c1) = row_ident_gpu(keys, col_descs); `rows` holds the smallest
    input row of every identity whose diffs do not sum to zero, identities
    in signed lexicographic (c0, c1) order, and `wsum` the sums.  Grouping
    by the identity itself, where the chain it replaces compared (key, value
    hash) among neighbours, differs only if two 128-bit hashes collide,
    which the engine rules out everywhere (the value hash is one).

    One device-to-host read: survivors and the overflow word of the prefix
    repair together.  On overflow (more than `max_run` rows share a 32-bit
    prefix of c0 and differ, or more than `max_dirty` such runs) the
    identities are grouped again by group_combine_gpu's 64-bit sort, with
    further reads."""
    lib = require_lib()
    n = keys.shape[0]
    dev = keys.device
    assert keys.dtype == torch.int64 and keys.dim() == 2 and keys.shape[1] == 2
    assert 2 <= n < 2**32
    assert 1 <= prefix_bits <= 32 and 2 <= max_run <= 3072
    assert 1 <= max_dirty < 2**32
    keys = keys.contiguous()
    diffs = diffs.contiguous()
    assert diffs.dtype == torch.int64 and diffs.shape == (n,)
    args, keep = _ri_args(col_descs, n, dev)
    nlo, nhi = _none_hash()
    nblocks = (n + 255) // 256
    # one scratch allocation, in int64 words: ckeys (2n), k0_sorted,
    # k1_sorted, first, sums (n each), block csum + ctl (nblocks + 4), then
    # the 32-bit arrays perm32 (n), dirty_list (max_dirty), block_counts
    h32 = lambda m: (m + 1) // 2
    sizes = [2 * n, n, n, n, n, nblocks + 4, h32(n), h32(max_dirty), h32(nblocks)]
    work = torch.empty(sum(sizes), dtype=torch.int64, device=dev)
    ckeys_flat, k0s, k1s, first, sums, csum_ctl, perm32, dirty_list, block_counts = (
        work.split(sizes)
    )
    ckeys = ckeys_flat.view(n, 2)
    ctl = csum_ctl[nblocks:]
    # the results are narrowed views of `out`: kept apart from the scratch,
    # which a result then does not keep alive
    out = torch.empty((4 if gather_keys else 2, n), dtype=torch.int64, device=dev)
    out_rows, out_w = out[0], out[1]
    out_keys = out[2:].view(n, 2) if gather_keys else None
    temp, tbytes = _gc_temp(lib, n, True, dev)
    lib.pw_consolidate_rows.restype = ctypes.c_int
    rc = lib.pw_consolidate_rows(
        ctypes.c_void_p(keys.data_ptr()),
        ctypes.c_int64(n),
        *args,
        ctypes.c_uint64(nlo),
        ctypes.c_uint64(nhi),
        ctypes.c_void_p(diffs.data_ptr()),
        ctypes.c_void_p(ckeys.data_ptr()),
        ctypes.c_void_p(temp.data_ptr()),
        ctypes.c_int64(tbytes),
        ctypes.c_void_p(k0s.data_ptr()),
        ctypes.c_void_p(k1s.data_ptr()),
        ctypes.c_void_p(perm32.data_ptr()),
        ctypes.c_int(prefix_bits),
        ctypes.c_int64(max_run),
        ctypes.c_int64(max_dirty),
        ctypes.c_void_p(dirty_list.data_ptr()),
        ctypes.c_void_p(ctl.data_ptr()),
        ctypes.c_void_p(block_counts.data_ptr()),
        ctypes.c_void_p(csum_ctl.data_ptr()),
        ctypes.c_void_p(first.data_ptr()),
        ctypes.c_void_p(sums.data_ptr()),
        ctypes.c_void_p(out_rows.data_ptr()),
        ctypes.c_void_p(out_w.data_ptr()),
        ctypes.c_void_p(out_keys.data_ptr() if gather_keys else None),
        _stream_ptr(),
    )
    if rc != 0:
        raise RuntimeError(f"pw_consolidate_rows failed: hip error {rc}")
    del keep
    overflow, _dirty, total, _nseg = ctl.tolist()
    consolidate_path_counts["fused"] += 1
    if overflow:
        consolidate_path_counts["overflow"] += 1
        _uk0, _uk1, rows, (wsum,) = group_combine_gpu(
            ckeys, [diffs], full_sort=True, bucket=False
        )
        nz = wsum.nonzero(as_tuple=True)[0]
        rows, wsum = rows.index_select(0, nz), wsum.index_select(0, nz)
        if gather_keys:
            return rows, wsum, keys.index_select(0, rows)
        return rows, wsum
    if gather_keys:
        return out_rows[:total], out_w[:total], out_keys[:total]
    return out_rows[:total], out_w[:total]


#: blocks of k_partition_count / k_partition_scatter at the most; each owns
#: one contiguous chunk of rows
PART_MAX_BLOCKS = 2048


def partition_gpu(dest: torch.Tensor, world: int) -> tuple[torch.Tensor, torch.Tensor]:
    """Radix partition by destination rank: returns (perm, counts) with rows
    grouped by destination (exchange shuffle pack; pact.rs:56 analog).

    dest is a 1-D int64 tensor and 1 <= world <= 64.  Every dest[i] must lie
    in [0, world): the kernels index a world-sized histogram with it
    unchecked, so a value outside that range is the caller's error.  The
    order of rows inside one destination is unspecified."""
    lib = require_lib()
    if world < 1:
        raise ValueError(f"partition_gpu needs world >= 1, got {world}")
    if dest.dtype != torch.int64:
        raise ValueError(f"partition_gpu needs int64 destinations, got {dest.dtype}")
    if dest.dim() != 1:
        raise ValueError(f"partition_gpu needs 1-D destinations, got {dest.dim()}-D")
    n = dest.shape[0]
    nblocks = max(1, min(PART_MAX_BLOCKS, (n + 255) // 256))
    perm = torch.empty(n, dtype=torch.int64, device=dest.device)
    counts = torch.empty(world, dtype=torch.int64, device=dest.device)
    scratch = torch.empty(nblocks * world, dtype=torch.int64, device=dest.device)
    dest = dest.contiguous()
    rc = lib.pw_partition(
        ctypes.c_void_p(dest.data_ptr()),
        ctypes.c_int64(n),
        ctypes.c_int(world),
        ctypes.c_void_p(perm.data_ptr()),
        ctypes.c_void_p(counts.data_ptr()),
        ctypes.c_void_p(scratch.data_ptr()),
        ctypes.c_int64(nblocks),
        _stream_ptr(),
    )
    if rc != 0:
        raise RuntimeError(f"pw_partition failed: hip error {rc}")
    return perm, counts


def gemm_bias_act_gpu(
    a: torch.Tensor,
    b_t: torch.Tensor,
    bias: torch.Tensor | None = None,
    act: str = "none",
) -> torch.Tensor:
    """Hand-written MFMA bf16 GEMM with fused bias(+GELU) epilogue.

    a (M,K) bf16, b_t = B^T (N,K) bf16 row-major (weights are static, so
    the transpose is one-time); bias (N,) float32; returns (M,N) bf16.
    mfma_f32_16x16x32_bf16 tiles, fp32 accumulate.
    """
    lib = require_lib()
    assert a.dtype == torch.bfloat16 and b_t.dtype == torch.bfloat16
    M, K = a.shape
    N, K2 = b_t.shape
    assert K == K2
    out = torch.empty((M, N), dtype=torch.bfloat16, device=a.device)
    if M == 0 or N == 0:
        return out  # nothing to compute, and a grid of no blocks is an error
    if bias is not None:
        bias = bias.to(torch.float32).contiguous()
    act_code = {"none": 0, "gelu": 1}[act]
    rc = lib.pw_gemm_bf16(
        ctypes.c_void_p(a.contiguous().data_ptr()),
        ctypes.c_void_p(b_t.contiguous().data_ptr()),
        ctypes.c_void_p(bias.data_ptr() if bias is not None else 0),
        ctypes.c_void_p(out.data_ptr()),
        ctypes.c_int64(M),
        ctypes.c_int64(N),
        ctypes.c_int64(K),
        ctypes.c_int(act_code),
        _stream_ptr(),
    )
    if rc != 0:
        raise RuntimeError(f"pw_gemm_bf16 failed: hip error {rc}")
    return out


def topk_gpu(scores: torch.Tensor, k: int) -> tuple[torch.Tensor, torch.Tensor]:
    """Per-row top-k (higher=better) via the hand-written HIP kernel.

    scores (nq, m) float32 -> (vals (nq, k) f32, idx (nq, k) int64),
    1 <= k <= 32, values non-increasing along a row.  A row with fewer
    than k scores above -inf leaves its last slots unfilled: (-inf, -1),
    the value torch.topk gives such a slot and an index no row has.  NaN
    scores are never selected.  Equal scores rank in no defined order.
    """
    lib = require_lib()
    nq, m = scores.shape
    assert scores.dtype == torch.float32
    vals = torch.empty((nq, k), dtype=torch.float32, device=scores.device)
    idx = torch.empty((nq, k), dtype=torch.int64, device=scores.device)
    if nq == 0:
        return vals, idx
    rc = lib.pw_topk(
        ctypes.c_void_p(scores.contiguous().data_ptr()),
        ctypes.c_int64(nq),
        ctypes.c_int64(m),
        ctypes.c_int(k),
        ctypes.c_void_p(vals.data_ptr()),
        ctypes.c_void_p(idx.data_ptr()),
        _stream_ptr(),
    )
    if rc != 0:
        raise RuntimeError(f"pw_topk failed: hip error {rc}")
    return vals, idx


#: doc slots per block of pw_bm25_score (PW_BM25_TILE in pw_kernels.hip);
#: tests size their corpora around it
BM25_TILE = 4096


def bm25_score(
    offsets: torch.Tensor,
    pidx: torch.Tensor,
    ptf: torch.Tensor,
    norm: torch.Tensor,
    q_off: torch.Tensor,
    q_term: torch.Tensor,
    q_idf: torch.Tensor,
    k1: float,
    pad_to: int = 1,
) -> torch.Tensor:
    """Okapi BM25 scores of a query batch over compiled CSR postings.

    offsets (V+1) int64, pidx (nnz) int32 doc slots ascending within each
    term, ptf (nnz) float32, norm (n) float32 = k1*(1-b+b*dl/avgdl); the
    batch in CSR form: q_off (Q+1) int32, q_term int32 (distinct term ids
    < V), q_idf float32.  Returns dense float32 scores (Q, n), where
    scores[q, d] = sum over q's terms of idf * tf*(k1+1) / (tf + norm[d]),
    summed in term order.  With pad_to > 1 the rows are padded with zeros
    to the next multiple of pad_to columns, so that a row splits into
    equal contiguous segments.

    CUDA tensors go through the pw_bm25_score kernel; CPU tensors run the
    same formula in torch (one float32 index_add_ per term), which is the
    CPU path and a second numerics reference for the kernel.
    """
    n = norm.shape[0]
    nq = q_off.shape[0] - 1
    assert offsets.dtype == torch.int64 and pidx.dtype == torch.int32
    assert ptf.dtype == torch.float32 and norm.dtype == torch.float32
    assert q_off.dtype == torch.int32 and q_term.dtype == torch.int32
    assert q_idf.dtype == torch.float32
    assert pidx.shape == ptf.shape and q_term.shape == q_idf.shape
    assert nq >= 0 and offsets.shape[0] >= 1
    k1p1 = float(k1) + 1.0
    n_pad = -(-n // pad_to) * pad_to
    if not norm.is_cuda:
        scores = torch.zeros((nq, n_pad), dtype=torch.float32)
        k1p1_t = torch.tensor(k1p1, dtype=torch.float32)
        qo = q_off.tolist()
        for q in range(nq):
            row = scores[q]
            for t in range(qo[q], qo[q + 1]):
                term = int(q_term[t])
                s, e = int(offsets[term]), int(offsets[term + 1])
                d = pidx[s:e].long()
                tf = ptf[s:e]
                row.index_add_(0, d, q_idf[t] * (tf * k1p1_t) / (tf + norm[d]))
        return scores
    lib = require_lib()
    assert BM25_TILE == lib.pw_bm25_tile(), "BM25_TILE out of step with the kernel"
    scores = torch.empty((nq, n_pad), dtype=torch.float32, device=norm.device)
    if n_pad > n:
        scores[:, n:] = 0.0
    rc = lib.pw_bm25_score(
        ctypes.c_void_p(offsets.contiguous().data_ptr()),
        ctypes.c_void_p(pidx.contiguous().data_ptr()),
        ctypes.c_void_p(ptf.contiguous().data_ptr()),
        ctypes.c_void_p(norm.contiguous().data_ptr()),
        ctypes.c_int64(n),
        ctypes.c_void_p(q_off.contiguous().data_ptr()),
        ctypes.c_void_p(q_term.contiguous().data_ptr()),
        ctypes.c_void_p(q_idf.contiguous().data_ptr()),
        ctypes.c_int64(nq),
        ctypes.c_float(k1p1),
        ctypes.c_void_p(scores.data_ptr()),
        ctypes.c_int64(n_pad),
        _stream_ptr(),
    )
    if rc != 0:
        raise RuntimeError(f"pw_bm25_score failed: hip error {rc}")
    return scores


def merge_consolidate_gpu(
    a_words: Sequence[torch.Tensor],
    a_accs: Sequence[torch.Tensor],
    b_words: Sequence[torch.Tensor],
    b_accs: Sequence[torch.Tensor],
    compare_words: int | None = None,
) -> tuple[list[torch.Tensor], list[torch.Tensor], torch.Tensor]:
    """Fused LSM merge+consolidate of two unique lex-sorted row sets.

    Rows are nw (<=4) int64 words; comparison uses the first
    `compare_words` (default all — pass 2 when the tail words are
    key-determined).  acc slot 0 is the weight; merged rows with zero
    weight are dropped.  Returns (out_words, accs, rep) with rep
    indexing concat([A, B]) rows (A preferred on matches) for
    carried-column gathers.
    """
    lib = require_lib()
    m = a_words[0].shape[0]
    n = b_words[0].shape[0]
    nw = len(a_words)
    nwc = compare_words or nw
    nacc = len(a_accs)
    assert len(b_accs) == nacc and 1 <= nacc <= 8 and 1 <= nwc <= nw <= 4
    device = a_words[0].device
    total_diag = m + n
    nthreads = max(1, (total_diag + 7) // 8)
    counts = torch.empty(nthreads, dtype=torch.int32, device=device)
    wA = [t.contiguous() for t in a_words]
    wB = [t.contiguous() for t in b_words]
    aA = [t.contiguous() for t in a_accs]
    aB = [t.contiguous() for t in b_accs]
    rc = lib.pw_merge_consolidate_count(
        _ptr_arr(wA),
        _ptr_arr(aA),
        _ptr_arr(wB),
        _ptr_arr(aB),
        ctypes.c_int(nw),
        ctypes.c_int(nwc),
        ctypes.c_int(nacc),
        ctypes.c_int64(m),
        ctypes.c_int64(n),
        ctypes.c_void_p(counts.data_ptr()),
        ctypes.c_int64(nthreads),
        _stream_ptr(),
    )
    if rc != 0:
        raise RuntimeError(f"pw_merge_consolidate_count failed: {rc}")
    csum = torch.cumsum(counts.to(torch.int64), 0)
    total = int(csum[-1].item())
    bases = torch.zeros(nthreads, dtype=torch.int64, device=device)
    bases[1:] = csum[:-1]
    out_words = [
        torch.empty(total, dtype=torch.int64, device=device)
        for _ in range(nw)
    ]
    out_accs = [
        torch.empty(total, dtype=torch.int64, device=device)
        for _ in range(nacc)
    ]
    rep = torch.empty(total, dtype=torch.int64, device=device)
    rc = lib.pw_merge_consolidate_emit(
        _ptr_arr(wA),
        _ptr_arr(aA),
        _ptr_arr(wB),
        _ptr_arr(aB),
        ctypes.c_int(nw),
        ctypes.c_int(nwc),
        ctypes.c_int(nacc),
        ctypes.c_int64(m),
        ctypes.c_int64(n),
        ctypes.c_void_p(bases.data_ptr()),
        ctypes.c_int64(nthreads),
        _ptr_arr(out_words),
        _ptr_arr(out_accs),
        ctypes.c_void_p(rep.data_ptr()),
        _stream_ptr(),
    )
    if rc != 0:
        raise RuntimeError(f"pw_merge_consolidate_emit failed: {rc}")
    return out_words, out_accs, rep


def group_update_gpu(
    a_words: Sequence[torch.Tensor],
    a_accs: Sequence[torch.Tensor],
    b_words: Sequence[torch.Tensor],
    b_accs: Sequence[torch.Tensor],
    out_slots: Sequence[int],
):
    """Merged state and emitted delta rows of a groupby-reduce step from
    one merge walk (pw_group_update_*).

    A (state) and B (consolidated delta) are unique lex-sorted 2-word row
    sets with 1..8 int64 accumulators, slot 0 the weight.  The state half
    is merge_consolidate_gpu's: (out_words, out_accs, rep).  The emitted
    half holds, for every B row whose output row changes, a retraction of
    the old row (old weight > 0) and an insertion of the new one (new
    weight > 0); a row is unchanged when both weights are positive and no
    slot of `out_slots` moves.  All retractions come first, then all
    insertions, each in B order: keys (n_out, 2), diffs (-1 / +1), one
    value tensor per slot of `out_slots` (in that order), and src, the
    row of concat([A, B]) holding the key's carried values.

    Returns (out_words, out_accs, rep, keys, diffs, vals, src).  One host
    sync (the three output sizes).
    """
    lib = require_lib()
    m = a_words[0].shape[0]
    n = b_words[0].shape[0]
    nacc = len(a_accs)
    assert len(a_words) == 2 and len(b_words) == 2
    assert len(b_accs) == nacc and 1 <= nacc <= 8
    slots = sorted(set(int(s) for s in out_slots))
    assert all(0 <= s < nacc for s in slots)
    mask = 0
    for s in slots:
        mask |= 1 << s
    device = b_words[0].device
    nthreads = max(1, (m + n + 7) // 8)
    counts = torch.empty(nthreads * 4, dtype=torch.int32, device=device)
    bases = torch.empty(nthreads * 3, dtype=torch.int64, device=device)
    totals = torch.empty(3, dtype=torch.int64, device=device)
    wA = [t.contiguous() for t in a_words]
    wB = [t.contiguous() for t in b_words]
    aA = [t.contiguous() for t in a_accs]
    aB = [t.contiguous() for t in b_accs]
    for t in wA + wB + aA + aB:
        assert t.dtype == torch.int64
    rc = lib.pw_group_update_count(
        _ptr_arr(wA),
        _ptr_arr(aA),
        _ptr_arr(wB),
        _ptr_arr(aB),
        ctypes.c_int(nacc),
        ctypes.c_uint(mask),
        ctypes.c_int64(m),
        ctypes.c_int64(n),
        ctypes.c_void_p(counts.data_ptr()),
        ctypes.c_void_p(bases.data_ptr()),
        ctypes.c_void_p(totals.data_ptr()),
        ctypes.c_int64(nthreads),
        _stream_ptr(),
    )
    if rc != 0:
        raise RuntimeError(f"pw_group_update_count failed: {rc}")
    n_keep, n_ret, n_ins = totals.tolist()  # the one host sync
    n_out = n_ret + n_ins

    def i64(k):
        return torch.empty(k, dtype=torch.int64, device=device)

    out_words = [i64(n_keep) for _ in range(2)]
    out_accs = [i64(n_keep) for _ in range(nacc)]
    rep = i64(n_keep)
    keys = torch.empty((n_out, 2), dtype=torch.int64, device=device)
    diffs = i64(n_out)
    vals = {s: i64(n_out) for s in slots}
    src = i64(n_out)
    varr = (ctypes.c_void_p * 8)(
        *[ctypes.c_void_p(vals[s].data_ptr() if s in vals else 0) for s in range(8)]
    )
    rc = lib.pw_group_update_emit(
        _ptr_arr(wA),
        _ptr_arr(aA),
        _ptr_arr(wB),
        _ptr_arr(aB),
        ctypes.c_int(nacc),
        ctypes.c_uint(mask),
        ctypes.c_int64(m),
        ctypes.c_int64(n),
        ctypes.c_void_p(bases.data_ptr()),
        ctypes.c_int64(n_ret),
        ctypes.c_int64(nthreads),
        _ptr_arr(out_words),
        _ptr_arr(out_accs),
        ctypes.c_void_p(rep.data_ptr()),
        ctypes.c_void_p(keys.data_ptr()),
        ctypes.c_void_p(diffs.data_ptr()),
        varr,
        ctypes.c_void_p(src.data_ptr()),
        _stream_ptr(),
    )
    if rc != 0:
        raise RuntimeError(f"pw_group_update_emit failed: {rc}")
    return out_words, out_accs, rep, keys, diffs, [vals[s] for s in slots], src


#: radix sort geometry: one wave of RS_LANES lanes per block, each lane a
#: contiguous chunk; RS_BLOCK_ROWS rows per block until RS_MAX_BLOCKS
#: blocks, longer chunks from there on
RS_LANES = 64
RS_BLOCK_ROWS = 64 * RS_LANES
RS_MAX_BLOCKS = 1024


def radix_sort64_gpu(keys: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """Hand-written LSD radix sort of int64 keys (signed order).

    Returns (sorted_keys, perm) with perm stable: equal keys keep their
    input order.  8x 8-bit digit passes; the (digit, block) scan runs as
    one torch cumsum between kernel launches.
    """
    lib = require_lib()
    n = keys.shape[0]
    device = keys.device
    perm = torch.arange(n, dtype=torch.int64, device=device)
    if n <= 1:
        return keys.clone(), perm
    nblocks = max(1, min(RS_MAX_BLOCKS, (n + RS_BLOCK_ROWS - 1) // RS_BLOCK_ROWS))
    chunk = (n + nblocks * RS_LANES - 1) // (nblocks * RS_LANES)
    ka = torch.empty(n, dtype=torch.int64, device=device)  # uint64 bits
    kb = torch.empty(n, dtype=torch.int64, device=device)
    pa = perm
    pb = torch.empty(n, dtype=torch.int64, device=device)
    keys = keys.contiguous()
    rc = lib.pw_radix_flip(
        ctypes.c_void_p(keys.data_ptr()),
        ctypes.c_void_p(ka.data_ptr()),
        ctypes.c_int64(n),
        _stream_ptr(),
    )
    if rc != 0:
        raise RuntimeError(f"pw_radix_flip failed: {rc}")
    counts = torch.empty(256 * nblocks, dtype=torch.int32, device=device)
    for p in range(8):
        shift = p * 8
        rc = lib.pw_radix_count(
            ctypes.c_void_p(ka.data_ptr()),
            ctypes.c_int64(n),
            ctypes.c_int(shift),
            ctypes.c_int64(nblocks),
            ctypes.c_int64(chunk),
            ctypes.c_void_p(counts.data_ptr()),
            _stream_ptr(),
        )
        if rc != 0:
            raise RuntimeError(f"pw_radix_count failed: {rc}")
        csum = torch.cumsum(counts.to(torch.int64), 0)
        bases = torch.zeros_like(csum)
        bases[1:] = csum[:-1]
        rc = lib.pw_radix_scatter(
            ctypes.c_void_p(ka.data_ptr()),
            ctypes.c_void_p(pa.data_ptr()),
            ctypes.c_int64(n),
            ctypes.c_int(shift),
            ctypes.c_int64(nblocks),
            ctypes.c_int64(chunk),
            ctypes.c_void_p(bases.data_ptr()),
            ctypes.c_void_p(kb.data_ptr()),
            ctypes.c_void_p(pb.data_ptr()),
            _stream_ptr(),
        )
        if rc != 0:
            raise RuntimeError(f"pw_radix_scatter failed: {rc}")
        ka, kb = kb, ka
        pa, pb = pb, pa
    out = torch.empty(n, dtype=torch.int64, device=device)
    rc = lib.pw_radix_unflip(
        ctypes.c_void_p(ka.data_ptr()),
        ctypes.c_void_p(out.data_ptr()),
        ctypes.c_int64(n),
        _stream_ptr(),
    )
    if rc != 0:
        raise RuntimeError(f"pw_radix_unflip failed: {rc}")
    return out, pa


def scan_positions_gpu(buf: torch.Tensor, target: int) -> torch.Tensor:
    """Ordered positions where buf == target (uint8 buffer) — the
    newline/separator scan of the ingest parse (replaces nonzero)."""
    lib = require_lib()
    n = buf.shape[0]
    device = buf.device
    nblocks = max(1, min(2048, (n + 4095) // 4096))
    counts = torch.empty(nblocks, dtype=torch.int64, device=device)
    rc = lib.pw_scan_positions(
        ctypes.c_void_p(buf.contiguous().data_ptr()),
        ctypes.c_int64(n),
        ctypes.c_int(int(target)),
        ctypes.c_void_p(counts.data_ptr()),
        ctypes.c_int64(nblocks),
        _stream_ptr(),
    )
    if rc != 0:
        raise RuntimeError(f"pw_scan_positions failed: {rc}")
    csum = torch.cumsum(counts, 0)
    total = int(csum[-1].item())
    bases = torch.zeros(nblocks, dtype=torch.int64, device=device)
    bases[1:] = csum[:-1]
    out = torch.empty(total, dtype=torch.int64, device=device)
    rc = lib.pw_scan_emit(
        ctypes.c_void_p(buf.contiguous().data_ptr()),
        ctypes.c_int64(n),
        ctypes.c_int(int(target)),
        ctypes.c_void_p(bases.data_ptr()),
        ctypes.c_int64(nblocks),
        ctypes.c_void_p(out.data_ptr()),
        _stream_ptr(),
    )
    if rc != 0:
        raise RuntimeError(f"pw_scan_emit failed: {rc}")
    return out


def sort_repair_gpu(
    k0_sorted: torch.Tensor,
    k1_sorted: torch.Tensor,
    perm: torch.Tensor,
    passes: int = 4,
) -> None:
    """In-place odd-even repair of word1 order inside equal-word0 runs
    (k_sort_repair) — the sync-free replacement for the 2-word sort fast
    path's collision check.  Mutates k1_sorted and perm.

    Contract: every equal-word0 run of up to `passes` rows ends up in
    ascending word1 order (odd-even transposition needs as many passes as
    the run has rows); a longer run may stay partly unordered.  The default
    of 4 repairs runs of up to 4 rows."""
    lib = require_lib()
    n = k0_sorted.shape[0]
    if n < 2:
        return
    rc = lib.pw_sort_repair(
        ctypes.c_void_p(k0_sorted.data_ptr()),
        ctypes.c_void_p(k1_sorted.data_ptr()),
        ctypes.c_void_p(perm.data_ptr()),
        ctypes.c_int64(n),
        ctypes.c_int(int(passes)),
        _stream_ptr(),
    )
    if rc != 0:
        raise RuntimeError(f"pw_sort_repair failed: hip error {rc}")


def gather_cols_gpu(idx: torch.Tensor, cols: list) -> list:
    """Gather up to 8 8-byte columns through one shared int64 index in a
    single launch (k_gather_cols) — replaces per-column index_select on
    the arrange/merge/consolidate permutation paths.  Columns with a
    non-8-byte itemsize fall back to torch indexing."""
    lib = require_lib()
    m = idx.shape[0]
    outs: list = [None] * len(cols)
    fused_pos: list[int] = []
    for i, c in enumerate(cols):
        if c.dim() == 1 and c.element_size() == 8 and c.is_contiguous():
            fused_pos.append(i)
        else:
            outs[i] = c[idx] if c.dim() > 1 else c.index_select(0, idx)
    idx = idx.contiguous()
    for start in range(0, len(fused_pos), 8):
        group = fused_pos[start : start + 8]
        srcs = (ctypes.c_void_p * len(group))()
        dsts = (ctypes.c_void_p * len(group))()
        for k, i in enumerate(group):
            c = cols[i]
            out = torch.empty(m, dtype=c.dtype, device=c.device)
            outs[i] = out
            srcs[k] = c.data_ptr()
            dsts[k] = out.data_ptr()
        rc = lib.pw_gather_cols(
            ctypes.c_void_p(idx.data_ptr()),
            ctypes.c_int64(m),
            ctypes.c_int(len(group)),
            srcs,
            dsts,
            _stream_ptr(),
        )
        if rc != 0:
            raise RuntimeError(f"pw_gather_cols failed: {rc}")
    return outs


def intern_error_message(e: int) -> str:
    """Text for the PW_HT_ERR_* bits of pw_kernels.hip."""
    parts = []
    if e & 1:
        parts.append("probe bound hit (table full)")
    if e & 2:
        parts.append("slot, claimer row or span out of range")
    if e & 4:
        parts.append("dictionary arrays or byte arena too small")
    return "device dictionary intern failed: " + "; ".join(parts or [str(e)])


def gather_spans_gpu(
    buf: torch.Tensor,
    starts: torch.Tensor,
    ends: torch.Tensor,
    first_rows: torch.Tensor,
    n_new: torch.Tensor,
    base: torch.Tensor,
    arena: torch.Tensor,
    cursor: torch.Tensor,
    tok_off: torch.Tensor,
    tok_len: torch.Tensor,
    err: torch.Tensor,
) -> None:
    """Pack the spans [starts[r], ends[r]) of rows r = first_rows[:n_new]
    of the uint8 `buf` into `arena` (k_gather_spans) and record each
    token's (offset, length) at code base+k.  n_new, base, cursor and err
    are 1-element int64 device tensors; nothing waits for the device."""
    lib = require_lib()
    nrows = starts.shape[0]
    if nrows == 0:
        return
    for t in (buf, starts, ends, first_rows, arena, tok_off, tok_len):
        assert t.is_contiguous()
    rc = lib.pw_gather_spans(
        ctypes.c_void_p(buf.data_ptr()),
        ctypes.c_int64(buf.shape[0]),
        ctypes.c_void_p(starts.data_ptr()),
        ctypes.c_void_p(ends.data_ptr()),
        ctypes.c_int64(nrows),
        ctypes.c_void_p(first_rows.data_ptr()),
        ctypes.c_void_p(n_new.data_ptr()),
        ctypes.c_void_p(base.data_ptr()),
        ctypes.c_void_p(arena.data_ptr()),
        ctypes.c_int64(arena.shape[0]),
        ctypes.c_void_p(cursor.data_ptr()),
        ctypes.c_void_p(tok_off.data_ptr()),
        ctypes.c_void_p(tok_len.data_ptr()),
        ctypes.c_int64(min(tok_off.shape[0], tok_len.shape[0])),
        ctypes.c_void_p(err.data_ptr()),
        _stream_ptr(),
    )
    if rc != 0:
        raise RuntimeError(f"pw_gather_spans failed: hip error {rc}")


#: int64 words per hash-table slot, (lo, hi, val, unused) — HT_SLOT_WORDS of
#: pw_kernels.hip
HT_SLOT_WORDS = 4


class DeviceHashTable:
    """Open-addressing device hash table over 128-bit keys -> int64 values
    (k_ht_build / k_ht_probe / k_ht_intern_*).  Build from a dictionary's
    hash arrays; probe per delta batch (closed world) or intern per delta
    batch (unseen keys are inserted).  Load factor <= 0.5 (nslots = next
    pow2 >= 2m).

    The table is one (nslots, HT_SLOT_WORDS) int64 tensor, `tab`; tab_lo,
    tab_hi and tab_val are its column views (shape (nslots,), strided), so
    in-place updates through them reach the table."""

    def __init__(self, klo: torch.Tensor, khi: torch.Tensor,
                 vals: torch.Tensor | None = None, reserve: int = 0):
        require_lib()
        m = klo.shape[0]
        device = klo.device
        self.nslots = self.slots_for(max(m, int(reserve)))
        #: OR of the PW_HT_ERR_* bits raised by the intern kernels (int64,
        #: 1 element; an owner may point it at a word of its own state)
        self.err = torch.zeros(1, dtype=torch.int64, device=device)
        self._alloc(device)
        self.insert(klo, khi, vals)

    @staticmethod
    def slots_for(m: int) -> int:
        """Smallest power-of-two slot count with load factor <= 0.5."""
        return 1 << max(4, (2 * m - 1).bit_length()) if m else 16

    def _alloc(self, device) -> None:
        if require_lib().pw_ht_slot_words() != HT_SLOT_WORDS:
            raise RuntimeError("libpwhip.so was built for another HT_SLOT_WORDS")
        self.tab = torch.full((self.nslots, HT_SLOT_WORDS), -1,
                              dtype=torch.int64, device=device)
        self.tab_lo = self.tab[:, 0]
        self.tab_hi = self.tab[:, 1]
        self.tab_val = self.tab[:, 2]

    def insert(self, klo: torch.Tensor, khi: torch.Tensor,
               vals: torch.Tensor | None = None) -> None:
        """pw_ht_build into the (possibly non-empty) table.  Keys must be
        unique and absent; the caller keeps the load factor <= 0.5."""
        lib = require_lib()
        m = klo.shape[0]
        if not m:
            return
        klo, khi = klo.contiguous(), khi.contiguous()
        vals = vals.contiguous() if vals is not None else None
        rc = lib.pw_ht_build(
            ctypes.c_void_p(klo.data_ptr()),
            ctypes.c_void_p(khi.data_ptr()),
            ctypes.c_void_p(vals.data_ptr()) if vals is not None else None,
            ctypes.c_int64(m),
            ctypes.c_void_p(self.tab.data_ptr()),
            ctypes.c_int64(self.nslots),
            _stream_ptr(),
        )
        if rc != 0:
            raise RuntimeError(f"pw_ht_build failed: hip error {rc}")

    def fits(self, size: int) -> bool:
        """True when `size` keys keep the load factor <= 0.5 — the bound
        the intern kernels' probe loops rely on."""
        return 2 * int(size) <= self.nslots

    def rebuild(self, size: int, klo: torch.Tensor, khi: torch.Tensor) -> None:
        """Re-hash into a table sized for `size` keys from the dictionary's
        hash arrays (row index == code)."""
        self.nslots = self.slots_for(max(int(size), klo.shape[0]))
        self._alloc(klo.device)
        self.insert(klo, khi, None)

    def intern(
        self,
        qlo: torch.Tensor,
        qhi: torch.Tensor,
        base,
        pool_lo: torch.Tensor,
        pool_hi: torch.Tensor,
        front: "DeviceHashTable | None" = None,
    ) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """Insert-or-get (k_ht_intern_*): returns (codes, first_rows, n_new).

        Known keys get their stored code; the batch's distinct new keys get
        base, base+1, ... in order of first occurrence by row index, are
        inserted, and their hashes written to pool_lo/pool_hi[base + k].
        `base` is the current dictionary size, an int or a 1-element int64
        device tensor (so a caller need not read it back).  first_rows[k]
        (k < n_new) is the row that introduced code base+k; n_new is a
        1-element device tensor — nothing here waits for the device.  The
        caller guarantees fits(size + n) and pool capacity >= size + n;
        violations raise bits in self.err instead of running out of bounds.

        `front` is an optional second table holding keys this one does not
        (a compact, cache-resident table of the keys known for certain):
        it is probed first and never written, and only its misses reach
        this table, which must be sized for a whole batch of new keys.
        """
        lib = require_lib()
        n = qlo.shape[0]
        device = qlo.device
        codes = torch.empty(n, dtype=torch.int64, device=device)
        first_rows = torch.empty(n, dtype=torch.int64, device=device)
        if n == 0:
            return codes, first_rows, torch.zeros(1, dtype=torch.int64, device=device)
        if not torch.is_tensor(base):
            base = torch.tensor([int(base)], dtype=torch.int64, device=device)
        assert base.dtype == torch.int64 and base.is_contiguous()
        assert pool_lo.is_contiguous() and pool_hi.is_contiguous()
        qlo, qhi = qlo.contiguous(), qhi.contiguous()
        # block counts and n_new share one allocation
        nblocks = max(1, min(2048, (n + 4095) // 4096))
        work = torch.empty(nblocks + 1, dtype=torch.int64, device=device)
        pend = torch.empty(n, dtype=torch.uint8, device=device)
        n_new = work[nblocks:]
        rc = lib.pw_ht_intern(
            ctypes.c_void_p(qlo.data_ptr()),
            ctypes.c_void_p(qhi.data_ptr()),
            ctypes.c_int64(n),
            ctypes.c_void_p(self.tab.data_ptr()),
            ctypes.c_int64(self.nslots),
            ctypes.c_void_p(front.tab.data_ptr() if front else None),
            ctypes.c_int64(front.nslots if front else 0),
            ctypes.c_void_p(base.data_ptr()),
            ctypes.c_void_p(pool_lo.data_ptr()),
            ctypes.c_void_p(pool_hi.data_ptr()),
            ctypes.c_int64(min(pool_lo.shape[0], pool_hi.shape[0])),
            ctypes.c_void_p(codes.data_ptr()),
            ctypes.c_void_p(pend.data_ptr()),
            ctypes.c_void_p(first_rows.data_ptr()),
            ctypes.c_void_p(work.data_ptr()),
            ctypes.c_int64(nblocks),
            ctypes.c_void_p(n_new.data_ptr()),
            ctypes.c_void_p(self.err.data_ptr()),
            _stream_ptr(),
        )
        if rc != 0:
            raise RuntimeError(f"pw_ht_intern failed: hip error {rc}")
        return codes, first_rows, n_new

    def check_error(self) -> None:
        """Blocking read of the intern kernels' error word."""
        e = int(self.err.item())
        if e:
            raise RuntimeError(intern_error_message(e))

    def probe(self, qlo: torch.Tensor, qhi: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
        """Returns (values, found); values are -1 where not found."""
        lib = require_lib()
        nq = qlo.shape[0]
        out = torch.empty(nq, dtype=torch.int64, device=qlo.device)
        found = torch.empty(nq, dtype=torch.bool, device=qlo.device)
        if nq == 0:
            return out, found
        rc = lib.pw_ht_probe(
            ctypes.c_void_p(qlo.contiguous().data_ptr()),
            ctypes.c_void_p(qhi.contiguous().data_ptr()),
            ctypes.c_int64(nq),
            ctypes.c_void_p(self.tab.data_ptr()),
            ctypes.c_int64(self.nslots),
            ctypes.c_void_p(out.data_ptr()),
            ctypes.c_void_p(found.data_ptr()),
            _stream_ptr(),
        )
        if rc != 0:
            raise RuntimeError(f"pw_ht_probe failed: hip error {rc}")
        return out, found


#: gather_all takes the fused kernel above this many index rows
GATHER_ALL_MIN_ROWS = 2048


def gather_all(idx: torch.Tensor, tensors: list) -> list:
    """Gather a list of same-length tensors through one index — fused
    k_gather_cols on device, per-tensor index_select elsewhere."""
    if (
        tensors
        and tensors[0].is_cuda
        and idx.shape[0] > GATHER_ALL_MIN_ROWS
        and lib_available()
    ):
        return gather_cols_gpu(idx, list(tensors))
    return [
        t.index_select(0, idx) if t.dim() == 1 else t[idx] for t in tensors
    ]
