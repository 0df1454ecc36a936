// pathway_amd HIP kernels for gfx950 (MI355X / CDNA4).
//
// Round-1 set:
//   * fused 128-bit row hashing (replaces ~60 chained torch int64 ops and
//     their launch overhead with one memory-bound pass)
//   * varlen byte-range hashing (strings: offsets+bytes arenas)
//   * fused consolidate-weights (segment boundary + weight segment-sum)
//   * sorted additive-state merge helper (count/sum reduce state)
//
// Design per /opt/skills/guides/cdna_hip_programming.md: 64-wide waves,
// 256-thread blocks, grid-stride loops capped near 2048 blocks for
// memory-bound kernels, coalesced 8B/lane accesses.  All launchers take the
// caller's hipStream_t (torch current stream) — no syncs inside.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include <cstring>  // rocprim.hpp uses std::memcpy without including it
#include <rocprim/rocprim.hpp>

#include "../xxhash_common.h"

#define PW_BLOCK 256
#define PW_MAX_GRID 2048

static inline int pw_grid(int64_t n) {
  int64_t g = (n + PW_BLOCK - 1) / PW_BLOCK;
  if (g > PW_MAX_GRID) g = PW_MAX_GRID;
  if (g < 1) g = 1;
  return (int)g;
}

// ---------------------------------------------------------------- hashing --

// up to 20 input word columns, SoA int64
struct WordPtrs {
  const uint64_t* p[20];
};

template <int W>
__global__ void k_hash128_words(WordPtrs ptrs, int64_t n, uint64_t* lo,
                                uint64_t* hi) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    uint64_t w[W];
#pragma unroll
    for (int j = 0; j < W; ++j) w[j] = ptrs.p[j][i];
    lo[i] = pw_xxh64_words<W>(w, PW_SEED_LO);
    hi[i] = pw_xxh64_words<W>(w, PW_SEED_HI);
  }
}

extern "C" int pw_hash128_words(const void** word_ptrs, int nwords, int64_t n,
                                void* lo, void* hi, void* stream) {
  WordPtrs ptrs;
  for (int j = 0; j < nwords && j < 20; ++j)
    ptrs.p[j] = (const uint64_t*)word_ptrs[j];
  hipStream_t s = (hipStream_t)stream;
  dim3 grid(pw_grid(n)), block(PW_BLOCK);
#define CASE(W)                                                        \
  case W:                                                              \
    hipLaunchKernelGGL((k_hash128_words<W>), grid, block, 0, s, ptrs,  \
                       n, (uint64_t*)lo, (uint64_t*)hi);               \
    break;
  switch (nwords) {
    CASE(1) CASE(2) CASE(3) CASE(4) CASE(5) CASE(6) CASE(7) CASE(8)
    CASE(9) CASE(10) CASE(11) CASE(12) CASE(13) CASE(14) CASE(15) CASE(16)
    CASE(17) CASE(18) CASE(19) CASE(20)
    default:
      return -1;
  }
#undef CASE
  return (int)hipGetLastError();
}

// tagged fixed-width value hash: hash of [tag, payload] per row
__global__ void k_value_hash(const uint64_t* payload, uint64_t tag, int64_t n,
                             uint64_t* lo, uint64_t* hi) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    uint64_t w[2] = {tag, payload[i]};
    lo[i] = pw_xxh64_words<2>(w, PW_SEED_LO);
    hi[i] = pw_xxh64_words<2>(w, PW_SEED_HI);
  }
}

extern "C" int pw_value_hash(const void* payload, uint64_t tag, int64_t n,
                             void* lo, void* hi, void* stream) {
  hipLaunchKernelGGL(k_value_hash, dim3(pw_grid(n)), dim3(PW_BLOCK), 0,
                     (hipStream_t)stream, (const uint64_t*)payload, tag, n,
                     (uint64_t*)lo, (uint64_t*)hi);
  return (int)hipGetLastError();
}

// varlen: hash of [tag-word || bytes[start:end]] per row, one row per
// thread per round.  pw_xxh64_tagged2 walks the row once for both seeds
// from aligned dword loads, entirely in registers (no staging buffer: a
// run-time indexed private array is spilled to LDS or scratch).  nbytes is
// the length of `bytes`; no load leaves [bytes, bytes + nbytes).
__global__ __launch_bounds__(PW_BLOCK) void k_varlen_hash(
    const uint8_t* __restrict__ bytes, int64_t nbytes,
    const int64_t* __restrict__ offsets, uint64_t tag, int64_t n,
    uint64_t* __restrict__ lo, uint64_t* __restrict__ hi) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t a = offsets[i], b = offsets[i + 1];
    const PwHash128 h = pw_xxh64_tagged2(bytes, nbytes, a, b - a, tag);
    lo[i] = h.lo;
    hi[i] = h.hi;
  }
}

extern "C" int pw_varlen_hash(const void* bytes, int64_t nbytes,
                              const void* offsets, uint64_t tag, int64_t n,
                              void* lo, void* hi, void* stream) {
  hipLaunchKernelGGL(k_varlen_hash, dim3(pw_grid(n)), dim3(PW_BLOCK), 0,
                     (hipStream_t)stream, (const uint8_t*)bytes, nbytes,
                     (const int64_t*)offsets, tag, n, (uint64_t*)lo,
                     (uint64_t*)hi);
  return (int)hipGetLastError();
}

// ------------------------------------------------------------ consolidate --

// fused: mark run starts over up-to-4 sorted word columns + inclusive-scan
// segment ids will still be done by torch cumsum; this kernel fuses the
// multi-column neq reduction (saves 2W-1 elementwise launches).
struct Words4 {
  const uint64_t* p[4];
};

__global__ void k_run_starts(Words4 w, int nw, int64_t n, bool* starts) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    bool ne = (i == 0);
    if (i > 0) {
      for (int j = 0; j < nw; ++j) ne |= (w.p[j][i] != w.p[j][i - 1]);
    }
    starts[i] = ne;
  }
}

extern "C" int pw_run_starts(const void** word_ptrs, int nwords, int64_t n,
                             void* starts, void* stream) {
  Words4 w;
  for (int j = 0; j < nwords && j < 4; ++j) w.p[j] = (const uint64_t*)word_ptrs[j];
  hipLaunchKernelGGL(k_run_starts, dim3(pw_grid(n)), dim3(PW_BLOCK), 0,
                     (hipStream_t)stream, w, nwords, n, (bool*)starts);
  return (int)hipGetLastError();
}

// ------------------------------------------------------------------- host --

extern "C" void pw_host_hash128_bytes(const void* data, int64_t n,
                                      uint64_t* lo, uint64_t* hi) {
  *lo = pw_xxh64_bytes((const uint8_t*)data, n, PW_SEED_LO);
  *hi = pw_xxh64_bytes((const uint8_t*)data, n, PW_SEED_HI);
}

// batch host hashing of varlen byte rows (string pool fills); the arena
// holds at least offsets[n] bytes
extern "C" void pw_host_varlen_hash(const void* bytes, const int64_t* offsets,
                                    uint64_t tag, int64_t n, uint64_t* lo,
                                    uint64_t* hi) {
  const uint8_t* b = (const uint8_t*)bytes;
  const int64_t nbytes = n > 0 ? offsets[n] : 0;
  for (int64_t i = 0; i < n; ++i) {
    const int64_t a = offsets[i], e = offsets[i + 1];
    const PwHash128 h = pw_xxh64_tagged2(b, nbytes, a, e - a, tag);
    lo[i] = h.lo;
    hi[i] = h.hi;
  }
}

// ------------------------------------------------------- sorted-key search --

// Lexicographic binary search over up-to-4 parallel sorted word columns.
// One thread per query — replaces the ~10-kernel-per-iteration torch
// binary-search loop (the dominant launch-overhead cost in the profile,
// profiles/wordcount_r01.md).
struct SWords {
  const uint64_t* s[4];
  const uint64_t* q[4];
};

__device__ __forceinline__ int pw_cmp_row(const SWords& w, int nw, int64_t si,
                                          int64_t qi) {
  // compare sorted[si] ? query[qi] as SIGNED int64 lexicographic
  for (int j = 0; j < nw; ++j) {
    int64_t a = (int64_t)w.s[j][si];
    int64_t b = (int64_t)w.q[j][qi];
    if (a < b) return -1;
    if (a > b) return 1;
  }
  return 0;
}

template <bool RIGHT>
__global__ void k_searchsorted(SWords w, int nw, int64_t m, int64_t nq,
                               int64_t* out) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nq;
       i += (int64_t)gridDim.x * blockDim.x) {
    int64_t lo = 0, hi = m;
    while (lo < hi) {
      int64_t mid = (lo + hi) >> 1;
      int c = pw_cmp_row(w, nw, mid, i);
      bool go_right = RIGHT ? (c <= 0) : (c < 0);
      if (go_right)
        lo = mid + 1;
      else
        hi = mid;
    }
    out[i] = lo;
  }
}

extern "C" int pw_searchsorted(const void** sorted_ptrs, const void** query_ptrs,
                               int nwords, int64_t m, int64_t nq, int right,
                               void* out, void* stream) {
  SWords w;
  for (int j = 0; j < nwords && j < 4; ++j) {
    w.s[j] = (const uint64_t*)sorted_ptrs[j];
    w.q[j] = (const uint64_t*)query_ptrs[j];
  }
  dim3 grid(pw_grid(nq)), block(PW_BLOCK);
  if (right)
    hipLaunchKernelGGL((k_searchsorted<true>), grid, block, 0,
                       (hipStream_t)stream, w, nwords, m, nq, (int64_t*)out);
  else
    hipLaunchKernelGGL((k_searchsorted<false>), grid, block, 0,
                       (hipStream_t)stream, w, nwords, m, nq, (int64_t*)out);
  return (int)hipGetLastError();
}

// lookup: left-searchsorted + equality check, fused (pos clamped, found flag)
__global__ void k_lookup(SWords w, int nw, int64_t m, int64_t nq, int64_t* pos,
                         bool* found) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nq;
       i += (int64_t)gridDim.x * blockDim.x) {
    int64_t lo = 0, hi = m;
    while (lo < hi) {
      int64_t mid = (lo + hi) >> 1;
      if (pw_cmp_row(w, nw, mid, i) < 0)
        lo = mid + 1;
      else
        hi = mid;
    }
    bool f = false;
    int64_t p = lo;
    if (lo < m && pw_cmp_row(w, nw, lo, i) == 0) f = true;
    if (p >= m) p = m > 0 ? m - 1 : 0;
    pos[i] = p;
    found[i] = f;
  }
}

extern "C" int pw_lookup(const void** sorted_ptrs, const void** query_ptrs,
                         int nwords, int64_t m, int64_t nq, void* pos,
                         void* found, void* stream) {
  SWords w;
  for (int j = 0; j < nwords && j < 4; ++j) {
    w.s[j] = (const uint64_t*)sorted_ptrs[j];
    w.q[j] = (const uint64_t*)query_ptrs[j];
  }
  hipLaunchKernelGGL(k_lookup, dim3(pw_grid(nq)), dim3(PW_BLOCK), 0,
                     (hipStream_t)stream, w, nwords, m, nq, (int64_t*)pos,
                     (bool*)found);
  return (int)hipGetLastError();
}

// key_range: lo (left bound) and hi (right bound) in one kernel
__global__ void k_key_range(SWords w, int nw, int64_t m, int64_t nq,
                            int64_t* lo_out, int64_t* hi_out) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nq;
       i += (int64_t)gridDim.x * blockDim.x) {
    int64_t lo = 0, hi = m;
    while (lo < hi) {
      int64_t mid = (lo + hi) >> 1;
      if (pw_cmp_row(w, nw, mid, i) < 0)
        lo = mid + 1;
      else
        hi = mid;
    }
    int64_t left = lo;
    lo = left;
    hi = m;
    while (lo < hi) {
      int64_t mid = (lo + hi) >> 1;
      if (pw_cmp_row(w, nw, mid, i) <= 0)
        lo = mid + 1;
      else
        hi = mid;
    }
    lo_out[i] = left;
    hi_out[i] = lo;
  }
}

extern "C" int pw_key_range(const void** sorted_ptrs, const void** query_ptrs,
                            int nwords, int64_t m, int64_t nq, void* lo,
                            void* hi, void* stream) {
  SWords w;
  for (int j = 0; j < nwords && j < 4; ++j) {
    w.s[j] = (const uint64_t*)sorted_ptrs[j];
    w.q[j] = (const uint64_t*)query_ptrs[j];
  }
  hipLaunchKernelGGL(k_key_range, dim3(pw_grid(nq)), dim3(PW_BLOCK), 0,
                     (hipStream_t)stream, w, nwords, m, nq, (int64_t*)lo,
                     (int64_t*)hi);
  return (int)hipGetLastError();
}

// ---------------------------------------------------- pooled string hash --

// Fused dictionary-column value hash: out = pool_hash[code] blended with
// the canonical None hash for code < 0.  Replaces a clamp + 2 gathers +
// 2 wheres + mask compare torch chain with one pass.
__global__ void k_pool_hash(const int64_t* codes, const uint64_t* pool_lo,
                            const uint64_t* pool_hi, uint64_t none_lo,
                            uint64_t none_hi, int64_t n, uint64_t* lo,
                            uint64_t* hi) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    int64_t c = codes[i];
    if (c >= 0) {
      lo[i] = pool_lo[c];
      hi[i] = pool_hi[c];
    } else {
      lo[i] = none_lo;
      hi[i] = none_hi;
    }
  }
}

extern "C" int pw_pool_hash(const void* codes, const void* pool_lo,
                            const void* pool_hi, uint64_t none_lo,
                            uint64_t none_hi, int64_t n, void* lo, void* hi,
                            void* stream) {
  hipLaunchKernelGGL(k_pool_hash, dim3(pw_grid(n)), dim3(PW_BLOCK), 0,
                     (hipStream_t)stream, (const int64_t*)codes,
                     (const uint64_t*)pool_lo, (const uint64_t*)pool_hi,
                     none_lo, none_hi, n, (uint64_t*)lo, (uint64_t*)hi);
  return (int)hipGetLastError();
}

// varlen hash with explicit [start, end) per row (token parse output —
// tokens exclude separators so rows are not contiguous); see k_varlen_hash
__global__ __launch_bounds__(PW_BLOCK) void k_varlen_hash_se(
    const uint8_t* __restrict__ bytes, int64_t nbytes,
    const int64_t* __restrict__ starts, const int64_t* __restrict__ ends,
    uint64_t tag, int64_t n, uint64_t* __restrict__ lo,
    uint64_t* __restrict__ hi) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t a = starts[i], b = ends[i];
    const PwHash128 h = pw_xxh64_tagged2(bytes, nbytes, a, b - a, tag);
    lo[i] = h.lo;
    hi[i] = h.hi;
  }
}

extern "C" int pw_varlen_hash_se(const void* bytes, int64_t nbytes,
                                 const void* starts, const void* ends,
                                 uint64_t tag, int64_t n, void* lo, void* hi,
                                 void* stream) {
  hipLaunchKernelGGL(k_varlen_hash_se, dim3(pw_grid(n)), dim3(PW_BLOCK), 0,
                     (hipStream_t)stream, (const uint8_t*)bytes, nbytes,
                     (const int64_t*)starts, (const int64_t*)ends, tag, n,
                     (uint64_t*)lo, (uint64_t*)hi);
  return (int)hipGetLastError();
}

// ------------------------------------------------------- hash aggregation --
//
// Sort-free per-batch pre-aggregation for additive group-reduce
// (count/int-sum): one pass over the batch accumulating into an open-
// addressing hash table keyed by the 128-bit group key, instead of
// radix-sorting the whole batch and running the segment-boundary chain
// (rocprof: sort family + partition/nonzero were ~0.9 ms of a 2.9 ms
// wordcount step at 4M rows).
//
// Claim protocol (no intra-wave spinning): CAS the first key word against
// EMPTY; the winner then publishes word1 and the representative row.  A
// reader that observes word0 == its key but an unpublished word1 simply
// mismatches and claims the next slot — the same key may transiently own
// two slots, which the (tiny) sorted consolidation of the collected
// uniques merges afterwards.  EMPTY is a reserved 64-bit value; group keys
// are xxh64 outputs, so a real key equals it with probability 2^-64.

#define PW_HA_EMPTY 0x8000000000000000ULL

struct AccPtrs {
  const long long* p[8];
};
struct AccPtrsMut {
  long long* p[8];
};

__global__ void k_hash_agg(const long long* k0, const long long* k1,
                           AccPtrs contribs, int nacc, int64_t n,
                           unsigned long long* tk0, long long* tk1,
                           AccPtrsMut taccs, long long* rep, uint64_t mask,
                           unsigned int* overflow) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    unsigned long long key0 = (unsigned long long)k0[i];
    long long key1 = k1[i];
    uint64_t slot = ((uint64_t)key0) & mask;
    // probe cap: the table is sized ~2x expected uniques (L2-resident);
    // a longer chain means the estimate was wrong -> flag and let the
    // caller redo the batch on the sort path with a bigger table
    for (uint64_t tries = 0; tries < 512 && tries <= mask; ++tries) {
      // plain load first: the overwhelmingly common case is an already
      // claimed, matching slot — an L2 read beats a CAS round-trip
      unsigned long long cur = tk0[slot];
      if (cur == PW_HA_EMPTY)
        cur = atomicCAS(&tk0[slot], PW_HA_EMPTY, key0);
      if (cur == PW_HA_EMPTY) {
        // claimed: publish the rest of the key + a representative row
        tk1[slot] = key1;
        rep[slot] = (long long)i;
        __threadfence();
      } else if (cur != key0) {
        slot = (slot + 1) & mask;
        continue;
      } else if (tk1[slot] != key1) {
        // word0 matches but word1 is different OR not yet published:
        // treat as mismatch and probe on (duplicate slots merge later)
        slot = (slot + 1) & mask;
        continue;
      }
      for (int a = 0; a < nacc; ++a)
        atomicAdd((unsigned long long*)&taccs.p[a][slot],
                  (unsigned long long)contribs.p[a][i]);
      goto next_row;
    }
    atomicOr(overflow, 1u);
  next_row:;
  }
}

__global__ void k_hash_agg_init(unsigned long long* tk0, uint64_t cap) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < cap;
       i += (uint64_t)gridDim.x * blockDim.x)
    tk0[i] = PW_HA_EMPTY;
}

__global__ void k_hash_agg_collect(const unsigned long long* tk0,
                                   const long long* tk1, AccPtrs taccs,
                                   const long long* rep, int nacc,
                                   uint64_t cap, unsigned int* counter,
                                   long long* out_k0, long long* out_k1,
                                   AccPtrsMut out_accs, long long* out_rep) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < cap;
       i += (uint64_t)gridDim.x * blockDim.x) {
    unsigned long long k = tk0[i];
    if (k == PW_HA_EMPTY) continue;
    unsigned int idx = atomicAdd(counter, 1u);
    out_k0[idx] = (long long)k;
    out_k1[idx] = tk1[i];
    out_rep[idx] = rep[i];
    for (int a = 0; a < nacc; ++a) out_accs.p[a][idx] = taccs.p[a][i];
  }
}

extern "C" int pw_hash_agg(const void* k0, const void* k1,
                           const void** contrib_ptrs, int nacc, int64_t n,
                           void* tk0, void* tk1, void** tacc_ptrs, void* rep,
                           int64_t capacity, void* counter, void* out_k0,
                           void* out_k1, void** out_acc_ptrs, void* out_rep,
                           void* overflow, void* stream) {
  if (nacc > 8) return 1;
  hipStream_t s = (hipStream_t)stream;
  AccPtrs cp;
  AccPtrsMut tp, op;
  for (int a = 0; a < nacc; ++a) {
    cp.p[a] = (const long long*)contrib_ptrs[a];
    tp.p[a] = (long long*)tacc_ptrs[a];
    op.p[a] = (long long*)out_acc_ptrs[a];
  }
  AccPtrs tpc;
  for (int a = 0; a < nacc; ++a) tpc.p[a] = tp.p[a];
  uint64_t mask = (uint64_t)capacity - 1;
  dim3 block(PW_BLOCK);
  hipLaunchKernelGGL(k_hash_agg_init, dim3(pw_grid(capacity)), block, 0, s,
                     (unsigned long long*)tk0, (uint64_t)capacity);
  hipLaunchKernelGGL(k_hash_agg, dim3(pw_grid(n)), block, 0, s,
                     (const long long*)k0, (const long long*)k1, cp, nacc, n,
                     (unsigned long long*)tk0, (long long*)tk1, tp,
                     (long long*)rep, mask, (unsigned int*)overflow);
  hipLaunchKernelGGL(k_hash_agg_collect, dim3(pw_grid(capacity)), block, 0, s,
                     (const unsigned long long*)tk0, (const long long*)tk1,
                     tpc, (long long*)rep, nacc, (uint64_t)capacity,
                     (unsigned int*)counter, (long long*)out_k0,
                     (long long*)out_k1, op, (long long*)out_rep);
  return (int)hipGetLastError();
}

// ------------------------------------------------------ fused seg-reduce --
//
// Replaces the segment-boundary chain of the sorted pre-aggregation
// (run-starts → cumsum → nonzero → gathers → per-acc prefix-sum diffs,
// ~15 small launches on a 4M-row batch) with two kernels + one tiny
// cumsum.  Input: rows sorted by the 2-word key; output: compacted unique
// keys, per-segment int64 sums for each accumulator, and the first-row
// index of every segment (the carried-column representative).
//
// K2 does a wave-level segmented sum (shfl_up over 64 lanes): one
// atomicAdd per run-per-wave instead of one per row — on sorted data with
// d duplicates per key that is a ~min(64, d)× reduction in atomics.

struct SegWords {
  const int64_t* p[8];
};

__global__ void k_segred_count(SegWords w, int nw, int64_t n,
                               int* block_counts) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int flag = 0;
  if (i < n) {
    if (i == 0) flag = 1;
    else {
      for (int j = 0; j < nw; ++j)
        if (w.p[j][i] != w.p[j][i - 1]) { flag = 1; break; }
    }
  }
  // block reduction of flags (blockDim = 256)
  __shared__ int cnt[PW_BLOCK / 64];
  int wavecnt = __popcll(__ballot(flag));
  if ((threadIdx.x & 63) == 0) cnt[threadIdx.x >> 6] = wavecnt;
  __syncthreads();
  if (threadIdx.x == 0) {
    int total = 0;
    for (int j = 0; j < PW_BLOCK / 64; ++j) total += cnt[j];
    block_counts[blockIdx.x] = total;
  }
}

__global__ void k_segred_emit(SegWords w, int nw, AccPtrs contribs, int nacc,
                              int64_t n, const long long* block_bases,
                              AccPtrsMut out_words, long long* out_first,
                              AccPtrsMut out_accs) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int lane = threadIdx.x & 63;
  int flag = 0;
  if (i < n) {
    if (i == 0) flag = 1;
    else {
      for (int j = 0; j < nw; ++j)
        if (w.p[j][i] != w.p[j][i - 1]) { flag = 1; break; }
    }
  }
  // block-wide exclusive scan of flags via per-wave ballot + LDS
  uint64_t ball = __ballot(flag);
  int wave = threadIdx.x >> 6;
  __shared__ int wave_tot[PW_BLOCK / 64];
  if (lane == 0) wave_tot[wave] = __popcll(ball);
  __syncthreads();
  int wave_base = 0;
  for (int j = 0; j < wave; ++j) wave_base += wave_tot[j];
  uint64_t below = ball & ((lane == 0) ? 0ULL : ((1ULL << lane) - 1));
  int local_excl = wave_base + __popcll(below);
  long long base = block_bases[blockIdx.x];
  // global segment id of row i (segments are 0-based); padding lanes get
  // the sentinel -1 so a real row followed by padding still detects its
  // run tail (dropping this cost the last segment whenever n % 64 != 0)
  long long sid = base + local_excl + flag - 1;
  if (i < n && flag) {
    for (int j = 0; j < nw; ++j) out_words.p[j][sid] = (long long)w.p[j][i];
    out_first[sid] = i;
  }
  // wave-segmented sums per accumulator
  long long s = (i < n) ? sid : -1;
  for (int a = 0; a < nacc; ++a) {
    long long v = (i < n) ? contribs.p[a][i] : 0;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      long long vv = __shfl_up(v, off, 64);
      long long ss = __shfl_up(s, off, 64);
      if (lane >= off && ss == s) v += vv;
    }
    long long nxt = __shfl_down(s, 1, 64);
    bool tail = (lane == 63) || (nxt != s);
    if (s >= 0 && tail)
      atomicAdd((unsigned long long*)&out_accs.p[a][s],
                (unsigned long long)v);
  }
}

extern "C" int pw_seg_reduce_count(const void** word_ptrs, int nw, int64_t n,
                                   void* block_counts, int64_t nblocks,
                                   void* stream) {
  if (nw > 8) return 1;
  SegWords w;
  for (int j = 0; j < nw; ++j) w.p[j] = (const int64_t*)word_ptrs[j];
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(k_segred_count, dim3((uint32_t)nblocks), dim3(PW_BLOCK),
                     0, s, w, nw, n, (int*)block_counts);
  return (int)hipGetLastError();
}

extern "C" int pw_seg_reduce_emit(const void** word_ptrs, int nw,
                                  const void** contrib_ptrs, int nacc,
                                  int64_t n, const void* block_bases,
                                  void** out_word_ptrs, void* out_first,
                                  void** out_acc_ptrs, int64_t nblocks,
                                  void* stream) {
  if (nacc > 8 || nw > 8) return 1;
  SegWords w;
  for (int j = 0; j < nw; ++j) w.p[j] = (const int64_t*)word_ptrs[j];
  AccPtrs cp;
  AccPtrsMut op, ow;
  for (int a = 0; a < nacc; ++a) {
    cp.p[a] = (const long long*)contrib_ptrs[a];
    op.p[a] = (long long*)out_acc_ptrs[a];
  }
  for (int j = 0; j < nw; ++j) ow.p[j] = (long long*)out_word_ptrs[j];
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(k_segred_emit, dim3((uint32_t)nblocks), dim3(PW_BLOCK),
                     0, s, w, nw, cp, nacc, n, (const long long*)block_bases,
                     ow, (long long*)out_first, op);
  return (int)hipGetLastError();
}

// ------------------------------------------------------------- partition --
// Radix partition of rows by destination rank (the exchange shuffle pack,
// reference pact.rs:56 / operators.rs:126).  dest[i] in [0, world);
// world <= 64.  Output: perm such that rows grouped by destination
// (sorted[j] = input[perm[j]]) and per-destination counts.  Order within a
// destination is unspecified (the exchange does not require stability).
//
// Two passes over dest, each block owning a contiguous chunk:
//   1. per-block histogram -> block_hist[b][d]
//   2. single-block exclusive scan in destination-major order gives each
//      (d, b) cell its global base
//   3. scatter: per-block shared counters (atomicAdd in LDS) assign
//      positions within the block's (d) quota.

#define PW_PART_MAX_DEST 64

__global__ void k_partition_count(const int64_t* dest, int64_t n,
                                  int64_t chunk, int world,
                                  long long* block_hist) {
  __shared__ int hist[PW_PART_MAX_DEST];
  for (int d = threadIdx.x; d < world; d += blockDim.x) hist[d] = 0;
  __syncthreads();
  int64_t start = (int64_t)blockIdx.x * chunk;
  int64_t end = min(start + chunk, n);
  for (int64_t i = start + threadIdx.x; i < end; i += blockDim.x)
    atomicAdd(&hist[(int)dest[i]], 1);
  __syncthreads();
  for (int d = threadIdx.x; d < world; d += blockDim.x)
    block_hist[(int64_t)blockIdx.x * world + d] = hist[d];
}

// exclusive scan over cells ordered (d major, b minor); also emits counts[d]
__global__ void k_partition_scan(long long* block_hist, int64_t nblocks,
                                 int world, long long* counts) {
  // single block; simple sequential scan (cells <= 64 * 4096)
  if (threadIdx.x == 0) {
    long long run = 0;
    for (int d = 0; d < world; ++d) {
      long long dtotal = 0;
      for (int64_t b = 0; b < nblocks; ++b) {
        long long c = block_hist[b * world + d];
        block_hist[b * world + d] = run;
        run += c;
        dtotal += c;
      }
      counts[d] = dtotal;
    }
  }
}

__global__ void k_partition_scatter(const int64_t* dest, int64_t n,
                                    int64_t chunk, int world,
                                    const long long* block_bases,
                                    int64_t* perm) {
  __shared__ unsigned int offs[PW_PART_MAX_DEST];
  for (int d = threadIdx.x; d < world; d += blockDim.x) offs[d] = 0;
  __syncthreads();
  int64_t start = (int64_t)blockIdx.x * chunk;
  int64_t end = min(start + chunk, n);
  const long long* base = block_bases + (int64_t)blockIdx.x * world;
  for (int64_t i = start + threadIdx.x; i < end; i += blockDim.x) {
    int d = (int)dest[i];
    unsigned int p = atomicAdd(&offs[d], 1u);
    perm[base[d] + p] = i;
  }
}

extern "C" int pw_partition(const void* dest, int64_t n, int world,
                            void* perm, void* counts, void* scratch,
                            int64_t nblocks, void* stream) {
  if (world > PW_PART_MAX_DEST) return 2;
  hipStream_t s = (hipStream_t)stream;
  int64_t chunk = (n + nblocks - 1) / nblocks;
  if (chunk < 1) chunk = 1;
  hipLaunchKernelGGL(k_partition_count, dim3((uint32_t)nblocks),
                     dim3(PW_BLOCK), 0, s, (const int64_t*)dest, n, chunk,
                     world, (long long*)scratch);
  hipLaunchKernelGGL(k_partition_scan, dim3(1), dim3(1), 0, s,
                     (long long*)scratch, nblocks, world,
                     (long long*)counts);
  hipLaunchKernelGGL(k_partition_scatter, dim3((uint32_t)nblocks),
                     dim3(PW_BLOCK), 0, s, (const int64_t*)dest, n, chunk,
                     world, (const long long*)scratch, (int64_t*)perm);
  return (int)hipGetLastError();
}

// ------------------------------------------------------------ MFMA GEMM --
// Hand-written bf16 GEMM on gfx950 matrix cores with fused bias +
// activation epilogue — the embedder's projection/FFN GEMMs (north-star:
// "embedder forward on bf16 MFMA tiles").  C (M,N) = A (M,K) x B (K,N),
// row-major bf16 inputs, fp32 accumulate via mfma_f32_16x16x32_bf16,
// bf16 store.  Block = 128x128 tile, 4 waves (2x2), each wave owns a
// 64x64 sub-tile = 4x4 fragments; K staged through LDS in BK=64 steps,
// double-buffered.  act: 0 = none, 1 = exact GELU.
//
// Fragment layouts (cdna_hip_programming.md §3, verified by the gpu test
// against torch fp32 matmul with asymmetric inputs):
//   A: lane holds A[row0 + (l&15)][k0 + (l>>4)*8 + j], j=0..7
//   B: lane holds B[k0 + (l>>4)*8 + j][col0 + (l&15)]
//   C/D: lane l reg r -> row = row0 + (l>>4)*4 + r, col = col0 + (l&15)

typedef __attribute__((ext_vector_type(8))) __bf16 pw_frag8;
typedef __attribute__((ext_vector_type(4))) float pw_frag4f;

#define PW_GEMM_BM 128
#define PW_GEMM_BN 128
#define PW_GEMM_BK 64

__device__ __forceinline__ float pw_gelu(float x) {
  return 0.5f * x * (1.0f + erff(x * 0.70710678118654752f));
}

// B is passed TRANSPOSED (Bt = B^T, (N, K) row-major): both A and Bt
// tiles then stage into LDS with linear 16B vector loads and both MFMA
// fragments are contiguous 8-element ds reads (weights are static, so
// the one-time transpose is free on the host side).
template <int NBUF>
__global__ __launch_bounds__(256) void k_gemm_bf16(
    const __bf16* __restrict__ A, const __bf16* __restrict__ Bt,
    const float* __restrict__ bias, __bf16* __restrict__ C, int64_t M,
    int64_t N, int64_t K, int act, int nbm) {
  // NBUF=2: classic intra-block double buffer (64 KB LDS, 2 blocks/CU).
  // NBUF=1: single buffer (32 KB LDS, ~5 blocks/CU) — latency hiding
  // from BLOCK-level parallelism instead; wins on short-K shapes where
  // the 6-iteration pipeline never fills (PMC: MfmaUtil 8.9% at NBUF=2).
  __shared__ __bf16 lasA[NBUF][PW_GEMM_BM][PW_GEMM_BK];
  // B stored TRANSPOSED in LDS ([col][k]) so each lane's 8-element
  // K-fragment is a contiguous ds_read_b128 (scattered writes happen
  // once per element; scattered reads would repeat per MFMA)
  __shared__ __bf16 lasBt[NBUF][PW_GEMM_BN][PW_GEMM_BK];
  // XCD-aware tile mapping: consecutive blockIdx tiles land on the same
  // XCD's L2 by swizzling in chunks (guide: blockIdx->tile must be
  // XCD-aware).  Simple bijective row-major with N-fastest is fine here
  // because N <= 12 tiles for the encoder shapes.
  int tile = blockIdx.x;
  int bm = tile % nbm;
  int bn = tile / nbm;
  int64_t row0 = (int64_t)bm * PW_GEMM_BM;
  int64_t col0 = (int64_t)bn * PW_GEMM_BN;
  int tid = threadIdx.x;
  int lane = tid & 63;
  int wave = tid >> 6;  // 0..3
  int wr = wave >> 1;   // wave row (0..1) -> 64-row strip
  int wc = wave & 1;    // wave col (0..1) -> 64-col strip

  pw_frag4f acc[4][4];
#pragma unroll
  for (int m = 0; m < 4; ++m)
#pragma unroll
    for (int n = 0; n < 4; ++n) acc[m][n] = {0.f, 0.f, 0.f, 0.f};

  int nk = (int)((K + PW_GEMM_BK - 1) / PW_GEMM_BK);
  bool interior_mn = (row0 + PW_GEMM_BM <= M) && (col0 + PW_GEMM_BN <= N);

  // fast staging for interior tiles: async global->LDS DMA, 16B per lane
  // (guide §5: global_load_lds dwordx4 — the compiler never auto-emits it).
  // Contract: only for K % 8 == 0, where every row of A and Bt, and every
  // 8-element chunk the DMA reads, is as aligned as the base pointer (16
  // bytes for a whole torch allocation).  Any other K leaves rows 2-, 4- or
  // 8-byte aligned and stages through load_tiles, whose vector loads fall
  // back to element loads at the K tail.
  auto load_tiles_gll = [&](int kt, int buf) {
    int64_t k0 = (int64_t)kt * PW_GEMM_BK;
    // A tile: 16 KiB = 16 wave-chunks of 1 KiB; 4 chunks per wave
    typedef const __attribute__((address_space(1))) uint8_t* gptr_t;
    typedef __attribute__((address_space(3))) uint8_t* lptr_t;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      int wchunk = wave * 4 + i;
      int eoff = wchunk * 512 + lane * 8;
      int r = eoff >> 6, c = eoff & 63;
      gptr_t srcA = (gptr_t)(const void*)&A[(row0 + r) * K + k0 + c];
      lptr_t dstA = (lptr_t)(void*)(&lasA[buf][0][0] + wchunk * 512);
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)srcA,
                                       (__attribute__((address_space(3))) void*)dstA,
                                       16, 0, 0);
      gptr_t srcB = (gptr_t)(const void*)&Bt[(col0 + r) * K + k0 + c];
      lptr_t dstB = (lptr_t)(void*)(&lasBt[buf][0][0] + wchunk * 512);
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)srcB,
                                       (__attribute__((address_space(3))) void*)dstB,
                                       16, 0, 0);
    }
  };

  // cooperative tile load: 256 threads, A tile 128x64 (8192 elems = 32/thread),
  // 8-wide vector loads -> 4 loads per thread
  auto load_tiles = [&](int kt, int buf) {
    int64_t k0 = (int64_t)kt * PW_GEMM_BK;
    // A: each thread loads 4 rows' 8-element chunks
    for (int it = tid; it < (PW_GEMM_BM * PW_GEMM_BK) / 8; it += 256) {
      int r = it / (PW_GEMM_BK / 8);
      int cchunk = it % (PW_GEMM_BK / 8);
      int64_t grow = row0 + r;
      int64_t gcol = k0 + cchunk * 8;
      __bf16* dst = &lasA[buf][r][cchunk * 8];
      if (grow < M && gcol + 8 <= K) {
        *(pw_frag8*)dst = *(const pw_frag8*)&A[grow * K + gcol];
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j)
          dst[j] = (grow < M && gcol + j < K) ? A[grow * K + gcol + j]
                                              : (__bf16)0.f;
      }
    }
    // Bt: tile 128 (N-rows) x 64 (K-cols), linear like A
    for (int it = tid; it < (PW_GEMM_BN * PW_GEMM_BK) / 8; it += 256) {
      int r = it / (PW_GEMM_BK / 8);
      int cchunk = it % (PW_GEMM_BK / 8);
      int64_t grow = col0 + r;       // N index
      int64_t gcol = k0 + cchunk * 8;  // K index
      __bf16* dst = &lasBt[buf][r][cchunk * 8];
      if (grow < N && gcol + 8 <= K) {
        *(pw_frag8*)dst = *(const pw_frag8*)&Bt[grow * K + gcol];
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j)
          dst[j] = (grow < N && gcol + j < K) ? Bt[grow * K + gcol + j]
                                              : (__bf16)0.f;
      }
    }
  };

  auto stage = [&](int kt, int buf) {
    if (interior_mn && (K & 7) == 0 && (int64_t)(kt + 1) * PW_GEMM_BK <= K)
      load_tiles_gll(kt, buf);
    else
      load_tiles(kt, buf);
  };
  stage(0, 0);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  for (int kt = 0; kt < nk; ++kt) {
    int buf = NBUF == 2 ? (kt & 1) : 0;
    if (NBUF == 2 && kt + 1 < nk) stage(kt + 1, buf ^ 1);
#pragma unroll
    for (int kk = 0; kk < PW_GEMM_BK / 32; ++kk) {
      // hoist every fragment read out of the MFMA loops: B re-read per m
      // was 4x the LDS traffic and the dominant bank-conflict source
      // (PMC: LdsBankConflict ratio 3.0 before, MfmaUtil 8.9%)
      int ak = kk * 32 + (lane >> 4) * 8;
      pw_frag8 afrag[4], bfrag[4];
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        int arow = wr * 64 + m * 16 + (lane & 15);
        afrag[m] = *(const pw_frag8*)&lasA[buf][arow][ak];
      }
#pragma unroll
      for (int n = 0; n < 4; ++n) {
        int bcol = wc * 64 + n * 16 + (lane & 15);
        bfrag[n] = *(const pw_frag8*)&lasBt[buf][bcol][ak];
      }
#pragma unroll
      for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int n = 0; n < 4; ++n)
          acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              afrag[m], bfrag[n], acc[m][n], 0, 0, 0);
    }
    if (NBUF == 2) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
    } else if (kt + 1 < nk) {
      __syncthreads();  // everyone done reading buf before overwrite
      stage(kt + 1, 0);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
    }
  }

  // epilogue: bias + activation, bf16 store
#pragma unroll
  for (int m = 0; m < 4; ++m) {
#pragma unroll
    for (int n = 0; n < 4; ++n) {
      int64_t col = col0 + wc * 64 + n * 16 + (lane & 15);
      if (col >= N) continue;
      float bv = bias ? bias[col] : 0.f;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        int64_t row = row0 + wr * 64 + m * 16 + (lane >> 4) * 4 + r;
        if (row >= M) continue;
        float v = acc[m][n][r] + bv;
        if (act == 1) v = pw_gelu(v);
        C[row * N + col] = (__bf16)v;
      }
    }
  }
}

extern "C" int pw_gemm_bf16(const void* A, const void* B, const void* bias,
                            void* C, int64_t M, int64_t N, int64_t K,
                            int act, void* stream) {
  int nbm = (int)((M + PW_GEMM_BM - 1) / PW_GEMM_BM);
  int nbn = (int)((N + PW_GEMM_BN - 1) / PW_GEMM_BN);
  hipStream_t s = (hipStream_t)stream;
  // short-K shapes (few BK iterations) run the single-buffer variant:
  // the 2-deep pipeline never fills at nk<=8, so 5-blocks/CU occupancy
  // hides latency better than intra-block double buffering
  if ((K + PW_GEMM_BK - 1) / PW_GEMM_BK <= 8)
    hipLaunchKernelGGL(k_gemm_bf16<1>, dim3((uint32_t)(nbm * nbn)), dim3(256),
                       0, s, (const __bf16*)A, (const __bf16*)B,
                       (const float*)bias, (__bf16*)C, M, N, K, act, nbm);
  else
    hipLaunchKernelGGL(k_gemm_bf16<2>, dim3((uint32_t)(nbm * nbn)), dim3(256),
                       0, s, (const __bf16*)A, (const __bf16*)B,
                       (const float*)bias, (__bf16*)C, M, N, K, act, nbm);
  return (int)hipGetLastError();
}

// ----------------------------------------------------------------- top-k --
// Per-query top-k over a (nq, m) score matrix (higher = better) — the
// KNN answer selection (north-star: "cosine top-k" hand-written;
// replaces torch.topk on the query path).  One block per query; each
// thread keeps a k-deep insertion list over its strided slice, lists are
// merged in LDS by k selection passes.  k <= 32.
//
// The "empty" value is -inf, as torch.topk would value a missing
// candidate: a slot the row could not fill (fewer than k scores above
// -inf) is written (-inf, -1).  Every comparison is a strict `>`, so a
// -inf or NaN score is never inserted or selected, and every finite score
// down to float32 lowest can be.  Equal scores rank in no defined order.

#define PW_TOPK_MAXK 32

__global__ __launch_bounds__(256) void k_topk(
    const float* __restrict__ scores, int64_t m, int k,
    float* __restrict__ out_vals, int64_t* __restrict__ out_idx) {
  const float NEG = -INFINITY;
  __shared__ float svals[256 * PW_TOPK_MAXK];
  __shared__ int sidx[256 * PW_TOPK_MAXK];
  int64_t q = blockIdx.x;
  const float* row = scores + q * m;
  int tid = threadIdx.x;
  float lv[PW_TOPK_MAXK];
  int li[PW_TOPK_MAXK];
#pragma unroll
  for (int j = 0; j < PW_TOPK_MAXK; ++j) {
    lv[j] = NEG;
    li[j] = -1;
  }
  for (int64_t i = tid; i < m; i += 256) {
    float v = row[i];
    if (v > lv[k - 1]) {
      // insertion into the local sorted-descending list
      int p = k - 1;
      while (p > 0 && lv[p - 1] < v) {
        lv[p] = lv[p - 1];
        li[p] = li[p - 1];
        --p;
      }
      lv[p] = v;
      li[p] = (int)i;
    }
  }
  for (int j = 0; j < k; ++j) {
    svals[tid * k + j] = lv[j];
    sidx[tid * k + j] = li[j];
  }
  __syncthreads();
  // selection: k passes; wave 0 finds the global max of the 256*k
  // candidates via wave reduction and invalidates it.  The barrier is
  // block-uniform (every thread executes it each pass).
  for (int sel = 0; sel < k; ++sel) {
    if (tid < 64) {
      float best = NEG;
      int bestpos = -1;
      for (int p = tid; p < 256 * k; p += 64) {
        float v = svals[p];
        if (v > best || (v == best && bestpos >= 0 && p < bestpos)) {
          best = v;
          bestpos = p;
        }
      }
      // wave argmax reduction (ties -> lower position for determinism)
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) {
        float ov = __shfl_down(best, off);
        int op = __shfl_down(bestpos, off);
        if (ov > best || (ov == best && op >= 0 &&
                          (bestpos < 0 || op < bestpos))) {
          best = ov;
          bestpos = op;
        }
      }
      if (tid == 0) {
        // bestpos >= 0 only for a candidate above -inf (strict `>` above)
        if (bestpos >= 0) {
          out_vals[q * k + sel] = best;
          out_idx[q * k + sel] = sidx[bestpos];
          svals[bestpos] = NEG;
        } else {
          out_vals[q * k + sel] = NEG;
          out_idx[q * k + sel] = -1;
        }
      }
    }
    __syncthreads();
  }
}

extern "C" int pw_topk(const void* scores, int64_t nq, int64_t m, int k,
                       void* out_vals, void* out_idx, void* stream) {
  if (k > PW_TOPK_MAXK || k < 1) return 2;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(k_topk, dim3((uint32_t)nq), dim3(256), 0, s,
                     (const float*)scores, m, k, (float*)out_vals,
                     (int64_t*)out_idx);
  return (int)hipGetLastError();
}

// ------------------------------------------------------------ BM25 score --
// Okapi BM25 over compiled CSR postings for a batch of queries: dense
// scores (nq, n) in rows of row_stride >= n floats, every one of the n
// elements of a row written (the pad beyond n is the caller's).  offsets
// (V+1) int64, pidx (nnz) int32 doc slots ASCENDING WITHIN EACH TERM, ptf
// (nnz) term frequencies, norm (n) = k1*(1-b+b*dl/avgdl).  The query
// batch is CSR too: q_off (nq+1) int32 into q_term (distinct known term
// ids, < V) and q_idf.
//
// Grid (ceil(n/TILE), nq).  A block owns TILE consecutive doc slots and
// keeps their accumulators in LDS (16 KiB).  Per term it binary-searches
// the sub-range of the term's postings that falls in its tile, and its
// threads stride over that sub-range.  Doc slots are unique within a
// term, so no two lanes add to one accumulator; a barrier separates the
// terms (the term count is per query, hence block-uniform).  No float
// atomics: each accumulator is summed by one thread per term, in term
// order, so the result is bitwise reproducible.  A block reads at most
// TILE postings per term whatever the term's document frequency.

#define PW_BM25_TILE 4096
#define PW_BM25_MAX_GRID_Y 65535

// first p in [lo, hi) with a[p] >= x (hi if none)
__device__ __forceinline__ int64_t bm25_lower_bound(
    const int* __restrict__ a, int64_t lo, int64_t hi, int x) {
  while (lo < hi) {
    int64_t mid = lo + ((hi - lo) >> 1);
    if (a[mid] < x) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(256) void k_bm25_score(
    const int64_t* __restrict__ offsets, const int* __restrict__ pidx,
    const float* __restrict__ ptf, const float* __restrict__ norm,
    const int* __restrict__ q_off, const int* __restrict__ q_term,
    const float* __restrict__ q_idf, float k1p1, int n, int64_t row_stride,
    float* __restrict__ scores) {
  __shared__ float acc[PW_BM25_TILE];
  const int tid = threadIdx.x;
  const int q = blockIdx.y;
  const int tile_lo = blockIdx.x * PW_BM25_TILE;  // < n < 2^31
  const int tile_n = min(PW_BM25_TILE, n - tile_lo);
  for (int i = tid; i < PW_BM25_TILE; i += 256) acc[i] = 0.0f;
  __syncthreads();
  const int t_end = q_off[q + 1];
  for (int t = q_off[q]; t < t_end; ++t) {
    const int term = q_term[t];
    const float idf = q_idf[t];
    const int64_t e = offsets[term + 1];
    const int64_t lo = bm25_lower_bound(pidx, offsets[term], e, tile_lo);
    // tile_lo + tile_n <= n fits an int
    const int64_t hi = bm25_lower_bound(pidx, lo, e, tile_lo + tile_n);
    for (int64_t p = lo + tid; p < hi; p += 256) {
      const int d = pidx[p];  // in [tile_lo, tile_lo + tile_n)
      const float tf = ptf[p];
      acc[d - tile_lo] += idf * (tf * k1p1) / (tf + norm[d]);
    }
    __syncthreads();
  }
  float* row = scores + (int64_t)q * row_stride + tile_lo;
  for (int i = tid; i < tile_n; i += 256) row[i] = acc[i];
}

extern "C" int pw_bm25_tile() { return PW_BM25_TILE; }

extern "C" int pw_bm25_score(const void* offsets, const void* pidx,
                             const void* ptf, const void* norm, int64_t n,
                             const void* q_off, const void* q_term,
                             const void* q_idf, int64_t nq, float k1p1,
                             void* scores, int64_t row_stride,
                             void* stream) {
  if (n < 0 || n >= ((int64_t)1 << 31) || nq < 0 || row_stride < n) return 2;
  if (n == 0 || nq == 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  uint32_t tiles = (uint32_t)((n + PW_BM25_TILE - 1) / PW_BM25_TILE);
  for (int64_t q0 = 0; q0 < nq; q0 += PW_BM25_MAX_GRID_Y) {
    int64_t qc = nq - q0 < PW_BM25_MAX_GRID_Y ? nq - q0 : PW_BM25_MAX_GRID_Y;
    hipLaunchKernelGGL(k_bm25_score, dim3(tiles, (uint32_t)qc), dim3(256), 0,
                       s, (const int64_t*)offsets, (const int*)pidx,
                       (const float*)ptf, (const float*)norm,
                       (const int*)q_off + q0, (const int*)q_term,
                       (const float*)q_idf, k1p1, (int)n, row_stride,
                       (float*)scores + q0 * row_stride);
  }
  return (int)hipGetLastError();
}

// --------------------------------------------------- merge-consolidate --
// Fused LSM merge of the additive-reduce state:
// two UNIQUE lex-sorted 128-bit-key row sets (state A, delta B) with
// int64 accumulators merge into unique sorted keys, accumulators summed
// on key matches, rows whose weight slot (acc 0) sums to zero dropped.
// Replaces the searchsorted-merge + gather + segmented-reduce + nonzero
// + gather chain (~10 kernels) with count + emit over merge-path
// partitions (per-thread diagonal chunks; matched pairs are owned by
// the A side, a range starting on the B half of a match skips it).
// rep[] returns each output row's source row (j in A, or m + i in B;
// A preferred on matches) for carried-column gathers.

struct McAcc {
  const long long* p[8];
};
struct McAccMut {
  long long* p[8];
};
struct McWords {
  const int64_t* p[4];
};
struct McWordsMut {
  int64_t* p[4];
};

// compare the first nwc words (lexicographic, signed)
__device__ __forceinline__ bool mc_le(McWords A, int64_t i, McWords B,
                                      int64_t j, int nwc) {
  for (int w = 0; w < nwc; ++w) {
    if (A.p[w][i] != B.p[w][j]) return A.p[w][i] < B.p[w][j];
  }
  return true;
}

__device__ __forceinline__ bool mc_eq(McWords A, int64_t i, McWords B,
                                      int64_t j, int nwc) {
  for (int w = 0; w < nwc; ++w)
    if (A.p[w][i] != B.p[w][j]) return false;
  return true;
}

__device__ int64_t mc_merge_path(McWords A, int64_t m, McWords B, int64_t n,
                                 int64_t d, int nwc) {
  int64_t lo = d > n ? d - n : 0;
  int64_t hi = d < m ? d : m;
  while (lo < hi) {
    int64_t mid = (lo + hi) >> 1;
    if (mc_le(A, mid, B, d - mid - 1, nwc))
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo;  // ai; bi = d - ai
}

#define PW_MC_CHUNK 8

// one walk function used by both phases: WRITE=false counts only.
// nw = words carried to the output; nwc (<= nw) = comparison prefix
// (callers guarantee the tail words are key-determined when nwc < nw).
template <bool WRITE>
__device__ void mc_walk(McWords A, McAcc accA, McWords B, McAcc accB,
                        int nw, int nwc, int nacc, int64_t m, int64_t n,
                        int64_t d0, int64_t d1, int* count_out,
                        int64_t base, McWordsMut O, McAccMut accO,
                        int64_t* rep) {
  int64_t ai = mc_merge_path(A, m, B, n, d0, nwc);
  int64_t bi = d0 - ai;
  int64_t d = d0;
  // skip rule: a range starting on the B half of a match
  if (d < d1 && bi < n && ai > 0 &&
      !(ai < m && mc_le(A, ai, B, bi, nwc))) {
    if (mc_eq(A, ai - 1, B, bi, nwc)) {
      ++bi;
      ++d;
    }
  }
  int cnt = 0;
  int64_t w = base;
  while (d < d1) {
    bool take_a = (bi >= n) || (ai < m && mc_le(A, ai, B, bi, nwc));
    if (take_a) {
      bool matched = (bi < n) && mc_eq(A, ai, B, bi, nwc);
      long long wsum = accA.p[0][ai] + (matched ? accB.p[0][bi] : 0ll);
      if (wsum != 0) {
        if (WRITE) {
          for (int k = 0; k < nw; ++k) O.p[k][w] = A.p[k][ai];
          for (int c = 0; c < nacc; ++c)
            accO.p[c][w] =
                accA.p[c][ai] + (matched ? accB.p[c][bi] : 0ll);
          rep[w] = ai;
          ++w;
        }
        ++cnt;
      }
      ++ai;
      ++d;
      if (matched) {
        ++bi;
        ++d;
      }
    } else {
      long long wsum = accB.p[0][bi];
      if (wsum != 0) {
        if (WRITE) {
          for (int k = 0; k < nw; ++k) O.p[k][w] = B.p[k][bi];
          for (int c = 0; c < nacc; ++c) accO.p[c][w] = accB.p[c][bi];
          rep[w] = m + bi;
          ++w;
        }
        ++cnt;
      }
      ++bi;
      ++d;
    }
  }
  if (!WRITE) *count_out = cnt;
}

__global__ void k_mc_count(McWords A, McAcc accA, McWords B, McAcc accB,
                           int nw, int nwc, int nacc, int64_t m, int64_t n,
                           int* thread_counts, int64_t nthreads) {
  int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= nthreads) return;
  int64_t total = m + n;
  int64_t d0 = t * PW_MC_CHUNK;
  int64_t d1 = min(d0 + PW_MC_CHUNK, total);
  McAccMut dummy{};
  McWordsMut wdummy{};
  mc_walk<false>(A, accA, B, accB, nw, nwc, nacc, m, n, d0, d1,
                 &thread_counts[t], 0, wdummy, dummy, nullptr);
}

__global__ void k_mc_emit(McWords A, McAcc accA, McWords B, McAcc accB,
                          int nw, int nwc, int nacc, int64_t m, int64_t n,
                          const int64_t* bases, int64_t nthreads,
                          McWordsMut O, McAccMut accO, int64_t* rep) {
  int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= nthreads) return;
  int64_t total = m + n;
  int64_t d0 = t * PW_MC_CHUNK;
  int64_t d1 = min(d0 + PW_MC_CHUNK, total);
  mc_walk<true>(A, accA, B, accB, nw, nwc, nacc, m, n, d0, d1, nullptr,
                bases[t], O, accO, rep);
}

extern "C" int pw_merge_consolidate_count(
    const void** wordsA, const void** accA, const void** wordsB,
    const void** accB, int nw, int nwc, int nacc, int64_t m, int64_t n,
    void* thread_counts, int64_t nthreads, void* stream) {
  if (nacc > 8 || nacc < 1 || nw > 4 || nwc > nw) return 2;
  McAcc A{}, B{};
  McWords WA{}, WB{};
  for (int c = 0; c < nacc; ++c) {
    A.p[c] = (const long long*)accA[c];
    B.p[c] = (const long long*)accB[c];
  }
  for (int k = 0; k < nw; ++k) {
    WA.p[k] = (const int64_t*)wordsA[k];
    WB.p[k] = (const int64_t*)wordsB[k];
  }
  hipStream_t s = (hipStream_t)stream;
  int64_t blocks = (nthreads + PW_BLOCK - 1) / PW_BLOCK;
  hipLaunchKernelGGL(k_mc_count, dim3((uint32_t)blocks), dim3(PW_BLOCK), 0,
                     s, WA, A, WB, B, nw, nwc, nacc, m, n,
                     (int*)thread_counts, nthreads);
  return (int)hipGetLastError();
}

extern "C" int pw_merge_consolidate_emit(
    const void** wordsA, const void** accA, const void** wordsB,
    const void** accB, int nw, int nwc, int nacc, int64_t m, int64_t n,
    const void* bases, int64_t nthreads, void** out_words, void** accO,
    void* rep, void* stream) {
  if (nacc > 8 || nacc < 1 || nw > 4 || nwc > nw) return 2;
  McAcc A{}, B{};
  McAccMut O{};
  McWords WA{}, WB{};
  McWordsMut WO{};
  for (int c = 0; c < nacc; ++c) {
    A.p[c] = (const long long*)accA[c];
    B.p[c] = (const long long*)accB[c];
    O.p[c] = (long long*)accO[c];
  }
  for (int k = 0; k < nw; ++k) {
    WA.p[k] = (const int64_t*)wordsA[k];
    WB.p[k] = (const int64_t*)wordsB[k];
    WO.p[k] = (int64_t*)out_words[k];
  }
  hipStream_t s = (hipStream_t)stream;
  int64_t blocks = (nthreads + PW_BLOCK - 1) / PW_BLOCK;
  hipLaunchKernelGGL(k_mc_emit, dim3((uint32_t)blocks), dim3(PW_BLOCK), 0,
                     s, WA, A, WB, B, nw, nwc, nacc, m, n,
                     (const int64_t*)bases, nthreads, WO, O, (int64_t*)rep);
  return (int)hipGetLastError();
}

// ------------------------------------------------------------ group update --
// The groupby-reduce step on top of the merge above: the same walk over
// unique-sorted state A and unique-sorted delta B (2-word keys) that
// writes the merged state also writes the emitted delta batch, so the
// two binary-search lookups (before and after the merge) and the
// gather / mask / compare / nonzero / index_select / cat chain behind
// them are not needed.  Every B row j is consumed by exactly one thread,
// which has in registers
//   old[c] = matched ? accA[c][ai] : 0        new[c] = old[c] + accB[c][j]
//   old_p = old[0] > 0                        new_p = new[0] > 0
//   unchanged = old_p && new_p && old[c] == new[c] for every exposed slot
// and emits a retraction (old values, diff -1) when old_p && !unchanged
// and an insertion (new values, diff +1) when new_p && !unchanged.  The
// emitted rows are all retractions, then all insertions, each in B order.
// src[] is the row of concat([A, B]) that holds the key's carried group
// values (ai when matched, else m + j).
//
// count (3 counts per thread) -> single-block exclusive scan (bases and
// the 3 totals) -> one host read of the totals -> emit.

struct GuOut {
  int64_t* words[2];   // new state keys
  long long* accs[8];  // new state accumulators
  int64_t* rep;        // new state row -> row of concat([A, B])
  int64_t* keys;       // emitted keys, interleaved (n_out, 2)
  int64_t* diffs;      // emitted diffs
  long long* vals[8];  // emitted values, exposed slots only
  int64_t* src;        // emitted row -> row of concat([A, B])
};

// per-thread counts / bases: kept state rows, retractions, insertions
#define PW_GU_KEEP 0
#define PW_GU_RET 1
#define PW_GU_INS 2

template <bool WRITE>
__device__ __forceinline__ void gu_brow(McAcc accA, McWords B, McAcc accB,
                                        int nacc, unsigned out_slots,
                                        int64_t m, bool matched, int64_t ai,
                                        int64_t bi, int* cnt, int64_t* w,
                                        const GuOut& O) {
  long long old0 = matched ? accA.p[0][ai] : 0ll;
  long long new0 = old0 + accB.p[0][bi];
  bool old_p = old0 > 0, new_p = new0 > 0;
  // old[c] == new[c] exactly when the delta of slot c is zero
  bool same = true;
  for (int c = 0; c < nacc; ++c)
    if (((out_slots >> c) & 1u) && accB.p[c][bi] != 0) same = false;
  bool unchanged = old_p && new_p && same;
  if (old_p && !unchanged) {  // old_p implies matched
    if (WRITE) {
      int64_t r = w[PW_GU_RET]++;
      O.keys[2 * r] = B.p[0][bi];
      O.keys[2 * r + 1] = B.p[1][bi];
      O.diffs[r] = -1;
      for (int c = 0; c < nacc; ++c)
        if ((out_slots >> c) & 1u) O.vals[c][r] = accA.p[c][ai];
      O.src[r] = ai;
    }
    ++cnt[PW_GU_RET];
  }
  if (new_p && !unchanged) {
    if (WRITE) {
      int64_t r = w[PW_GU_INS]++;
      O.keys[2 * r] = B.p[0][bi];
      O.keys[2 * r + 1] = B.p[1][bi];
      O.diffs[r] = 1;
      for (int c = 0; c < nacc; ++c)
        if ((out_slots >> c) & 1u)
          O.vals[c][r] = (matched ? accA.p[c][ai] : 0ll) + accB.p[c][bi];
      O.src[r] = matched ? ai : m + bi;
    }
    ++cnt[PW_GU_INS];
  }
}

// mc_walk with nw = nwc = 2 plus the per-B-row emission.  w[] holds the
// three write cursors (WRITE only); cnt[] returns the three counts.
template <bool WRITE>
__device__ void gu_walk(McWords A, McAcc accA, McWords B, McAcc accB,
                        int nacc, unsigned out_slots, int64_t m, int64_t n,
                        int64_t d0, int64_t d1, int* cnt, int64_t* w,
                        const GuOut& O) {
  int64_t ai = mc_merge_path(A, m, B, n, d0, 2);
  int64_t bi = d0 - ai;
  int64_t d = d0;
  // skip rule: a range starting on the B half of a match
  if (d < d1 && bi < n && ai > 0 &&
      !(ai < m && mc_le(A, ai, B, bi, 2))) {
    if (mc_eq(A, ai - 1, B, bi, 2)) {
      ++bi;
      ++d;
    }
  }
  while (d < d1) {
    bool take_a = (bi >= n) || (ai < m && mc_le(A, ai, B, bi, 2));
    if (take_a) {
      bool matched = (bi < n) && mc_eq(A, ai, B, bi, 2);
      long long wsum = accA.p[0][ai] + (matched ? accB.p[0][bi] : 0ll);
      if (wsum != 0) {
        if (WRITE) {
          int64_t r = w[PW_GU_KEEP]++;
          O.words[0][r] = A.p[0][ai];
          O.words[1][r] = A.p[1][ai];
          for (int c = 0; c < nacc; ++c)
            O.accs[c][r] = accA.p[c][ai] + (matched ? accB.p[c][bi] : 0ll);
          O.rep[r] = ai;
        }
        ++cnt[PW_GU_KEEP];
      }
      if (matched) {
        gu_brow<WRITE>(accA, B, accB, nacc, out_slots, m, true, ai, bi, cnt,
                       w, O);
        ++bi;
        ++d;
      }
      ++ai;
      ++d;
    } else {
      long long wsum = accB.p[0][bi];
      if (wsum != 0) {
        if (WRITE) {
          int64_t r = w[PW_GU_KEEP]++;
          O.words[0][r] = B.p[0][bi];
          O.words[1][r] = B.p[1][bi];
          for (int c = 0; c < nacc; ++c) O.accs[c][r] = accB.p[c][bi];
          O.rep[r] = m + bi;
        }
        ++cnt[PW_GU_KEEP];
      }
      gu_brow<WRITE>(accA, B, accB, nacc, out_slots, m, false, ai, bi, cnt, w,
                     O);
      ++bi;
      ++d;
    }
  }
}

// thread_counts: (nthreads, 4) int32 — keep, retract, insert, pad
__global__ void k_gu_count(McWords A, McAcc accA, McWords B, McAcc accB,
                           int nacc, unsigned out_slots, int64_t m, int64_t n,
                           int4* thread_counts, int64_t nthreads) {
  int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= nthreads) return;
  int64_t d0 = t * PW_MC_CHUNK;
  int64_t d1 = min(d0 + PW_MC_CHUNK, m + n);
  int cnt[3] = {0, 0, 0};
  GuOut none{};
  gu_walk<false>(A, accA, B, accB, nacc, out_slots, m, n, d0, d1, cnt,
                 nullptr, none);
  thread_counts[t] = make_int4(cnt[0], cnt[1], cnt[2], 0);
}

// Exclusive scan of the three per-thread counts in one block: tiles of
// THREADS * ITEMS threads' counts, int32 inside a tile (a thread counts at
// most PW_MC_CHUNK rows of each kind), int64 carry across tiles.
// bases: (nthreads, 3) int64; totals: 3 int64.
#define PW_GU_SCAN_THREADS 1024
#define PW_GU_SCAN_ITEMS 4

__global__ __launch_bounds__(PW_GU_SCAN_THREADS) void k_gu_scan(
    const int4* thread_counts, int64_t nthreads, int64_t* bases,
    int64_t* totals) {
  __shared__ int wave_tot[PW_GU_SCAN_THREADS / 64][3];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  long long carry[3] = {0, 0, 0};
  const int64_t tile = (int64_t)PW_GU_SCAN_THREADS * PW_GU_SCAN_ITEMS;
  for (int64_t t0 = 0; t0 < nthreads; t0 += tile) {
    int64_t first = t0 + (int64_t)tid * PW_GU_SCAN_ITEMS;
    int v[PW_GU_SCAN_ITEMS][3];
    int sum[3] = {0, 0, 0};
#pragma unroll
    for (int k = 0; k < PW_GU_SCAN_ITEMS; ++k) {
      int4 c = make_int4(0, 0, 0, 0);
      if (first + k < nthreads) c = thread_counts[first + k];
      v[k][0] = c.x;
      v[k][1] = c.y;
      v[k][2] = c.z;
      sum[0] += c.x;
      sum[1] += c.y;
      sum[2] += c.z;
    }
    int incl[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      int x = sum[a];
      for (int dlt = 1; dlt < 64; dlt <<= 1) {
        int y = __shfl_up(x, dlt, 64);
        if (lane >= dlt) x += y;
      }
      incl[a] = x;
      if (lane == 63) wave_tot[wave][a] = x;
    }
    __syncthreads();
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      int before = 0, all = 0;
      for (int wv = 0; wv < PW_GU_SCAN_THREADS / 64; ++wv) {
        int wt = wave_tot[wv][a];
        if (wv < wave) before += wt;
        all += wt;
      }
      long long run = carry[a] + before + incl[a] - sum[a];
#pragma unroll
      for (int k = 0; k < PW_GU_SCAN_ITEMS; ++k) {
        if (first + k < nthreads) bases[(first + k) * 3 + a] = run;
        run += v[k][a];
      }
      carry[a] += all;
    }
    __syncthreads();
  }
  if (tid < 3) totals[tid] = carry[tid];
}

__global__ void k_gu_emit(McWords A, McAcc accA, McWords B, McAcc accB,
                          int nacc, unsigned out_slots, int64_t m, int64_t n,
                          const int64_t* bases, int64_t n_ret,
                          int64_t nthreads, GuOut O) {
  int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= nthreads) return;
  int64_t d0 = t * PW_MC_CHUNK;
  int64_t d1 = min(d0 + PW_MC_CHUNK, m + n);
  int cnt[3] = {0, 0, 0};
  int64_t w[3] = {bases[t * 3 + PW_GU_KEEP], bases[t * 3 + PW_GU_RET],
                  n_ret + bases[t * 3 + PW_GU_INS]};
  gu_walk<true>(A, accA, B, accB, nacc, out_slots, m, n, d0, d1, cnt, w, O);
}

static void gu_args(const void** wordsA, const void** accA,
                    const void** wordsB, const void** accB, int nacc,
                    McWords* WA, McAcc* A, McWords* WB, McAcc* B) {
  for (int c = 0; c < nacc; ++c) {
    A->p[c] = (const long long*)accA[c];
    B->p[c] = (const long long*)accB[c];
  }
  for (int k = 0; k < 2; ++k) {
    WA->p[k] = (const int64_t*)wordsA[k];
    WB->p[k] = (const int64_t*)wordsB[k];
  }
}

// count + scan: thread_counts (nthreads, 4) int32 scratch, bases
// (nthreads, 3) int64, totals 3 int64 (state rows, retractions, insertions)
extern "C" int pw_group_update_count(
    const void** wordsA, const void** accA, const void** wordsB,
    const void** accB, int nacc, unsigned out_slots, int64_t m, int64_t n,
    void* thread_counts, void* bases, void* totals, int64_t nthreads,
    void* stream) {
  if (nacc > 8 || nacc < 1 || nthreads < 1) return 2;
  McAcc A{}, B{};
  McWords WA{}, WB{};
  gu_args(wordsA, accA, wordsB, accB, nacc, &WA, &A, &WB, &B);
  hipStream_t s = (hipStream_t)stream;
  int64_t blocks = (nthreads + PW_BLOCK - 1) / PW_BLOCK;
  hipLaunchKernelGGL(k_gu_count, dim3((uint32_t)blocks), dim3(PW_BLOCK), 0, s,
                     WA, A, WB, B, nacc, out_slots, m, n,
                     (int4*)thread_counts, nthreads);
  hipLaunchKernelGGL(k_gu_scan, dim3(1), dim3(PW_GU_SCAN_THREADS), 0, s,
                     (const int4*)thread_counts, nthreads, (int64_t*)bases,
                     (int64_t*)totals);
  return (int)hipGetLastError();
}

// out_vals[c] is read for the slots of out_slots only
extern "C" int pw_group_update_emit(
    const void** wordsA, const void** accA, const void** wordsB,
    const void** accB, int nacc, unsigned out_slots, int64_t m, int64_t n,
    const void* bases, int64_t n_ret, int64_t nthreads, void** out_words,
    void** out_accs, void* rep, void* out_keys, void* out_diffs,
    void** out_vals, void* src, void* stream) {
  if (nacc > 8 || nacc < 1 || nthreads < 1) return 2;
  McAcc A{}, B{};
  McWords WA{}, WB{};
  gu_args(wordsA, accA, wordsB, accB, nacc, &WA, &A, &WB, &B);
  GuOut O{};
  for (int k = 0; k < 2; ++k) O.words[k] = (int64_t*)out_words[k];
  for (int c = 0; c < nacc; ++c) {
    O.accs[c] = (long long*)out_accs[c];
    if ((out_slots >> c) & 1u) O.vals[c] = (long long*)out_vals[c];
  }
  O.rep = (int64_t*)rep;
  O.keys = (int64_t*)out_keys;
  O.diffs = (int64_t*)out_diffs;
  O.src = (int64_t*)src;
  hipStream_t s = (hipStream_t)stream;
  int64_t blocks = (nthreads + PW_BLOCK - 1) / PW_BLOCK;
  hipLaunchKernelGGL(k_gu_emit, dim3((uint32_t)blocks), dim3(PW_BLOCK), 0, s,
                     WA, A, WB, B, nacc, out_slots, m, n,
                     (const int64_t*)bases, n_ret, nthreads, O);
  return (int)hipGetLastError();
}

// -------------------------------------------------------------- radix sort --
// Hand-written LSD radix sort of int64 keys with an int64 payload (the
// permutation) — the mandated sort kernel for the 128-bit key path
// (lex_sort_words' primary-word sort; the k1 tiebreak remains the
// existing duplicate-check).  Signed order = unsigned order after the
// sign bit is flipped once on input (flipped back on output).
//
// Per 8-bit digit pass:
//   k_rs_count: one wave per block, each lane owns a contiguous chunk
//     and counts serially (stable) into its LDS row; rows reduce to
//     per-(block,digit) counts, laid out digit-major for the scan.
//   <scan over (digit, block) runs in torch: one cumsum>
//   k_rs_scatter: lanes re-walk their chunks; position = scanned base
//     for (digit, block) + prefix of earlier lanes' counts (serial
//     per-digit LDS prefix) + running in-lane count.

#define PW_RS_THREADS 64
#define PW_RS_DIGITS 256

__global__ __launch_bounds__(PW_RS_THREADS) void k_rs_flip(
    const int64_t* in, uint64_t* out, int64_t n, int dir) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x)
    out[i] = (uint64_t)in[i] ^ 0x8000000000000000ull;
}

__global__ __launch_bounds__(PW_RS_THREADS) void k_rs_count(
    const uint64_t* keys, int64_t n, int shift, int64_t chunk,
    int* block_digit_counts /* [DIGITS][nblocks] digit-major */,
    int64_t nblocks) {
  __shared__ int cnt[PW_RS_THREADS][PW_RS_DIGITS];
  int lane = threadIdx.x;
  for (int d = 0; d < PW_RS_DIGITS; ++d) cnt[lane][d] = 0;
  int64_t start = ((int64_t)blockIdx.x * PW_RS_THREADS + lane) * chunk;
  int64_t end = min(start + chunk, n);
  for (int64_t i = start; i < end; ++i) {
    int d = (int)((keys[i] >> shift) & 0xFF);
    ++cnt[lane][d];
  }
  __syncthreads();
  // reduce lanes per digit: lane handles digits lane, lane+64, ...
  for (int d = lane; d < PW_RS_DIGITS; d += PW_RS_THREADS) {
    int s = 0;
    for (int t = 0; t < PW_RS_THREADS; ++t) s += cnt[t][d];
    block_digit_counts[(int64_t)d * nblocks + blockIdx.x] = s;
  }
}

__global__ __launch_bounds__(PW_RS_THREADS) void k_rs_scatter(
    const uint64_t* keys, const int64_t* payload, int64_t n, int shift,
    int64_t chunk, const long long* bases /* [DIGITS][nblocks] excl */,
    int64_t nblocks, uint64_t* out_keys, int64_t* out_payload) {
  // counts accumulate into lane_base, then convert to exclusive prefix
  // in place (one LDS array keeps us under the 160 KB/CU limit)
  __shared__ long long lane_base[PW_RS_THREADS][PW_RS_DIGITS];
  int lane = threadIdx.x;
  for (int d = 0; d < PW_RS_DIGITS; ++d) lane_base[lane][d] = 0;
  int64_t start = ((int64_t)blockIdx.x * PW_RS_THREADS + lane) * chunk;
  int64_t end = min(start + chunk, n);
  for (int64_t i = start; i < end; ++i) {
    int d = (int)((keys[i] >> shift) & 0xFF);
    ++lane_base[lane][d];
  }
  __syncthreads();
  // serial exclusive prefix over lanes per digit (lane d' handles
  // digits d', d'+64, ...)
  for (int d = lane; d < PW_RS_DIGITS; d += PW_RS_THREADS) {
    long long run = bases[(int64_t)d * nblocks + blockIdx.x];
    for (int t = 0; t < PW_RS_THREADS; ++t) {
      long long c = lane_base[t][d];
      lane_base[t][d] = run;
      run += c;
    }
  }
  __syncthreads();
  for (int64_t i = start; i < end; ++i) {
    int d = (int)((keys[i] >> shift) & 0xFF);
    long long p = lane_base[lane][d]++;
    out_keys[p] = keys[i];
    out_payload[p] = payload[i];
  }
}

__global__ __launch_bounds__(PW_RS_THREADS) void k_rs_unflip(
    const uint64_t* in, int64_t* out, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x)
    out[i] = (int64_t)(in[i] ^ 0x8000000000000000ull);
}

extern "C" int pw_radix_flip(const void* in, void* out, int64_t n,
                             void* stream) {
  hipStream_t s = (hipStream_t)stream;
  int64_t blocks = min((int64_t)2048, (n + PW_RS_THREADS - 1) / PW_RS_THREADS);
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL(k_rs_flip, dim3((uint32_t)blocks), dim3(PW_RS_THREADS),
                     0, s, (const int64_t*)in, (uint64_t*)out, n, 0);
  return (int)hipGetLastError();
}

extern "C" int pw_radix_unflip(const void* in, void* out, int64_t n,
                               void* stream) {
  hipStream_t s = (hipStream_t)stream;
  int64_t blocks = min((int64_t)2048, (n + PW_RS_THREADS - 1) / PW_RS_THREADS);
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL(k_rs_unflip, dim3((uint32_t)blocks),
                     dim3(PW_RS_THREADS), 0, s, (const uint64_t*)in,
                     (int64_t*)out, n);
  return (int)hipGetLastError();
}

extern "C" int pw_radix_count(const void* keys, int64_t n, int shift,
                              int64_t nblocks, int64_t chunk, void* counts,
                              void* stream) {
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(k_rs_count, dim3((uint32_t)nblocks),
                     dim3(PW_RS_THREADS), 0, s, (const uint64_t*)keys, n,
                     shift, chunk, (int*)counts, nblocks);
  return (int)hipGetLastError();
}

extern "C" int pw_radix_scatter(const void* keys, const void* payload,
                                int64_t n, int shift, int64_t nblocks,
                                int64_t chunk, const void* bases,
                                void* out_keys, void* out_payload,
                                void* stream) {
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(k_rs_scatter, dim3((uint32_t)nblocks),
                     dim3(PW_RS_THREADS), 0, s, (const uint64_t*)keys,
                     (const int64_t*)payload, n, shift, chunk,
                     (const long long*)bases, nblocks, (uint64_t*)out_keys,
                     (int64_t*)out_payload);
  return (int)hipGetLastError();
}

// ------------------------------------------------------------ mask scan --
// Ordered positions of matching bytes / true mask entries — the newline
// scan of the ingest parse and the run-start extraction, replacing
// rocprim partition (torch nonzero) with a count + emit pair whose scan
// is one torch cumsum.

// 16-bit hit mask of `target` inside the 16-byte granule at byte offset g.
// Vector path requires 16B alignment of buf+g (the host wrapper rounds the
// per-block chunk to a multiple of 16 and torch allocations are 256B-aligned,
// so interior granules qualify); the tail / unaligned path is scalar.
__device__ __forceinline__ unsigned pw_granule_mask(const uint8_t* buf,
                                                    int64_t g, int64_t end,
                                                    uint8_t t, bool aligned) {
  unsigned m = 0;
  if (aligned && g + 16 <= end) {
    uint4 v = *(const uint4*)(buf + g);
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (((w[q] >> (8 * j)) & 0xFFu) == t) m |= 1u << (4 * q + j);
  } else {
    for (int j = 0; j < 16 && g + j < end; ++j)
      if (buf[g + j] == t) m |= 1u << j;
  }
  return m;
}

__global__ void k_scan_count(const uint8_t* buf, int64_t n, int target,
                             int64_t chunk, long long* block_counts) {
  __shared__ int cnt;
  if (threadIdx.x == 0) cnt = 0;
  __syncthreads();
  int64_t start = (int64_t)blockIdx.x * chunk;
  int64_t end = min(start + chunk, n);
  const bool aligned = (((size_t)buf & 15) == 0);
  int local = 0;
  for (int64_t tile = start; tile < end; tile += (int64_t)blockDim.x * 16) {
    int64_t g = tile + (int64_t)threadIdx.x * 16;
    if (g < end)
      local += __popc(pw_granule_mask(buf, g, end, (uint8_t)target, aligned));
  }
  atomicAdd(&cnt, local);
  __syncthreads();
  if (threadIdx.x == 0) block_counts[blockIdx.x] = cnt;
}

__global__ void k_scan_emit(const uint8_t* buf, int64_t n, int target,
                            int64_t chunk, const long long* bases,
                            int64_t* out) {
  // Ordered emit: each 256-thread block walks its chunk in 4 KB tiles
  // (one 16 B granule per lane).  Per tile: wave-level __shfl_up inclusive
  // scan of per-granule hit counts + a 4-entry cross-wave prefix in LDS —
  // 2 barriers per 4 KB instead of a 16-barrier log-scan per 256 B.
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  __shared__ long long cursor;
  __shared__ int wave_tot[PW_BLOCK / 64];
  if (threadIdx.x == 0) cursor = bases[blockIdx.x];
  __syncthreads();
  int64_t start = (int64_t)blockIdx.x * chunk;
  int64_t end = min(start + chunk, n);
  const bool aligned = (((size_t)buf & 15) == 0);
  for (int64_t tile = start; tile < end; tile += (int64_t)blockDim.x * 16) {
    int64_t g = tile + (int64_t)threadIdx.x * 16;
    unsigned hmask =
        (g < end) ? pw_granule_mask(buf, g, end, (uint8_t)target, aligned) : 0u;
    int hits = __popc(hmask);
    int incl = hits;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      int v = __shfl_up(incl, off, 64);
      if (lane >= off) incl += v;
    }
    if (lane == 63) wave_tot[wave] = incl;
    __syncthreads();
    int wbase = 0;
    for (int w = 0; w < wave; ++w) wbase += wave_tot[w];
    long long my = cursor + wbase + (incl - hits);
    while (hmask) {
      int j = __ffs(hmask) - 1;
      hmask &= hmask - 1;
      out[my++] = g + j;
    }
    __syncthreads();
    if (threadIdx.x == (int)blockDim.x - 1) cursor += wbase + incl;
    __syncthreads();
  }
}

extern "C" int pw_scan_positions(const void* buf, int64_t n, int target,
                                 void* block_counts, int64_t nblocks,
                                 void* stream) {
  hipStream_t s = (hipStream_t)stream;
  int64_t chunk = ((n + nblocks - 1) / nblocks + 15) & ~(int64_t)15;
  if (chunk < 16) chunk = 16;
  hipLaunchKernelGGL(k_scan_count, dim3((uint32_t)nblocks), dim3(PW_BLOCK),
                     0, s, (const uint8_t*)buf, n, target,
                     chunk, (long long*)block_counts);
  return (int)hipGetLastError();
}

extern "C" int pw_scan_emit(const void* buf, int64_t n, int target,
                            const void* bases, int64_t nblocks, void* out,
                            void* stream) {
  hipStream_t s = (hipStream_t)stream;
  int64_t chunk = ((n + nblocks - 1) / nblocks + 15) & ~(int64_t)15;
  if (chunk < 16) chunk = 16;
  hipLaunchKernelGGL(k_scan_emit, dim3((uint32_t)nblocks), dim3(PW_BLOCK),
                     0, s, (const uint8_t*)buf, n, target, chunk,
                     (const long long*)bases, (int64_t*)out);
  return (int)hipGetLastError();
}

// ------------------------------------------------------- sort repair --
// After the 2-word fast-path sort by word0 only, rows in an equal-word0
// run may be out of order on word1.  Host-sync-checking for collisions
// cost 0.27 ms/step (10 syncs); instead: odd-even transposition passes
// restricted to equal-k0 pairs, entirely on device.  Contract: odd-even
// transposition sorts a run of L rows in L passes (wherever the run
// starts), so a call repairs every run of up to `passes` rows and may
// leave a longer one partly ordered.  The wrapper's default is 4 passes:
// with 64-bit hash keys a run of 5 needs five rows to share word0, about
// n^5 / 2^256 over n rows.  Signed compare matches torch.sort / the
// multi-pass fallback.

__global__ void k_sort_repair(const long long* __restrict__ k0,
                              long long* k1, long long* perm, int64_t n,
                              int parity) {
  int64_t i = 2 * ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) + parity;
  if (i + 1 >= n) return;
  if (k0[i] != k0[i + 1]) return;
  long long a = k1[i], b = k1[i + 1];
  if (a > b) {
    k1[i] = b;
    k1[i + 1] = a;
    long long p = perm[i];
    perm[i] = perm[i + 1];
    perm[i + 1] = p;
  }
}

extern "C" int pw_sort_repair(const void* k0, void* k1, void* perm,
                              int64_t n, int passes, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  int64_t pairs = n / 2 + 1;
  int64_t nblocks = (pairs + PW_BLOCK - 1) / PW_BLOCK;
  if (nblocks < 1) nblocks = 1;
  for (int p = 0; p < passes; ++p)
    hipLaunchKernelGGL(k_sort_repair, dim3((uint32_t)nblocks), dim3(PW_BLOCK),
                       0, s, (const long long*)k0, (long long*)k1,
                       (long long*)perm, n, p & 1);
  return (int)hipGetLastError();
}

// ------------------------------------------------------- fused gather --
// One launch gathers up to 8 8-byte columns through a shared index: the
// arrange/merge/consolidate paths gather (key words, weights, value
// columns) with the same permutation, and per-column index_select pays
// the index read + launch overhead k times.  Pointer table passed by
// value in the kernel args.

struct PwGather8 {
  const long long* src[8];
  long long* dst[8];
};

__global__ void k_gather_cols(const long long* __restrict__ idx, int64_t m,
                              int ncols, PwGather8 p) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < m; i += stride) {
    long long j = idx[i];
#pragma unroll 8
    for (int c = 0; c < 8; ++c) {
      if (c >= ncols) break;
      p.dst[c][i] = p.src[c][j];
    }
  }
}

// ------------------------------------------------------ hash table --
// Open-addressing (linear probe) device hash table over 128-bit keys —
// O(1) replacement for the binary-search k_lookup on hot stable
// dictionaries (the string-pool decode probes 4M tokens/step against a
// 50k vocab: ~1.2 slot loads beat a 16-level dependent-load search).
// Values are int64 >= 0; slot value -1 means empty.  Build never reads
// keys (inputs are unique), so a single atomicCAS on the value slot
// claims it.
//
// Layout: one int64 array of nslots slots of HT_SLOT_WORDS words each,
// (lo, hi, val, unused).  With 4 words a slot is 32 bytes and never
// straddles a cache line, so a probed slot costs one line where three
// parallel arrays cost three; the key pair is one 16-byte load and the
// value one 8-byte load, issued together.  All kernels address the table
// through PwHt; the Python side (ops.HT_SLOT_WORDS) mirrors the one
// constant.  val stays 8-byte aligned for the atomics.

#define HT_SLOT_WORDS 4
// independent queries per thread of k_ht_probe (1, 2 and 4 were measured,
// profiles/wordcount_r11.md)
#define PW_HT_PROBE_Q 2
#define HT_WORD_VAL 2

extern "C" int pw_ht_slot_words() { return HT_SLOT_WORDS; }

struct PwHtKey {
  long long lo, hi;
};

static_assert(HT_SLOT_WORDS % 2 == 0, "16-byte key loads need even slots");

struct PwHt {
  long long* w;
  __device__ __forceinline__ long long* slot(uint64_t s) const {
    return w + s * HT_SLOT_WORDS;
  }
  __device__ __forceinline__ long long* val(uint64_t s) const {
    return slot(s) + HT_WORD_VAL;
  }
  __device__ __forceinline__ PwHtKey key(uint64_t s) const {
    // slots are 16-byte aligned: one 16-byte load
    const longlong2 v = *(const longlong2*)slot(s);
    PwHtKey k;
    k.lo = v.x, k.hi = v.y;
    return k;
  }
  __device__ __forceinline__ void set_key(uint64_t s, long long lo,
                                          long long hi) const {
    longlong2 v;
    v.x = lo, v.y = hi;
    *(longlong2*)slot(s) = v;
  }
};

__global__ void k_ht_build(const int64_t* __restrict__ klo,
                           const int64_t* __restrict__ khi,
                           const int64_t* __restrict__ vals, int64_t m,
                           PwHt tab, int64_t mask) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < m; i += stride) {
    uint64_t slot = (uint64_t)klo[i] & (uint64_t)mask;
    while (atomicCAS((unsigned long long*)tab.val(slot),
                     (unsigned long long)(long long)-1,
                     (unsigned long long)(long long)(vals ? vals[i] : i)) !=
           (unsigned long long)(long long)-1)
      slot = (slot + 1) & (uint64_t)mask;
    tab.set_key(slot, klo[i], khi[i]);
  }
}

// Read-only probe of one key (the front table of k_ht_intern_claim): the
// stored value, or -1.  A slot's key and value are loaded together and
// tested afterwards (one trip to L2 per probed slot).  At most max_probes
// slots are examined.
__device__ __forceinline__ long long pw_ht_find(const PwHt tab, uint64_t mask,
                                                long long lo, long long hi,
                                                int64_t max_probes) {
  uint64_t slot = (uint64_t)lo & mask;
  for (int64_t probes = 0; probes < max_probes; ++probes) {
    const PwHtKey k = tab.key(slot);
    const long long tv = *tab.val(slot);
    if (tv < 0) return -1;  // empty -> miss
    if (k.lo == lo && k.hi == hi) return tv;
    slot = (slot + 1) & mask;
  }
  return -1;
}

__global__ __launch_bounds__(PW_BLOCK) void k_ht_probe(
    const int64_t* __restrict__ qlo, const int64_t* __restrict__ qhi,
    int64_t nq, const PwHt tab, int64_t mask, int64_t* __restrict__ out,
    bool* __restrict__ found) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  // PW_HT_PROBE_Q independent queries per thread; every round issues the
  // slot loads (key pair and value) of all of them, then tests.  As in the
  // front-table walk of k_ht_intern_claim, any negative value ends a walk
  // as a miss (-1 empty, <= -2 a pending slot left by a flagged intern
  // error), and a walk stops after nslots probes (a full table).
  for (; i < nq; i += stride * PW_HT_PROBE_Q) {
    long long lo[PW_HT_PROBE_Q], hi[PW_HT_PROBE_Q], v[PW_HT_PROBE_Q];
    uint64_t slot[PW_HT_PROBE_Q];
    bool live[PW_HT_PROBE_Q];
    bool any = false;
#pragma unroll
    for (int q = 0; q < PW_HT_PROBE_Q; ++q) {
      const int64_t j = i + q * stride;
      live[q] = j < nq;
      lo[q] = live[q] ? qlo[j] : 0;
      hi[q] = live[q] ? qhi[j] : 0;
      slot[q] = (uint64_t)lo[q] & (uint64_t)mask;
      v[q] = -1;
      any |= live[q];
    }
    for (int64_t probes = 0; any && probes <= mask; ++probes) {
      PwHtKey k[PW_HT_PROBE_Q];
      long long tv[PW_HT_PROBE_Q];
#pragma unroll
      for (int q = 0; q < PW_HT_PROBE_Q; ++q)
        if (live[q]) {
          k[q] = tab.key(slot[q]);
          tv[q] = *tab.val(slot[q]);
        }
      any = false;
#pragma unroll
      for (int q = 0; q < PW_HT_PROBE_Q; ++q)
        if (live[q]) {
          if (tv[q] < 0) {
            live[q] = false;
          } else if (k[q].lo == lo[q] && k[q].hi == hi[q]) {
            v[q] = tv[q];
            live[q] = false;
          } else {
            slot[q] = (slot[q] + 1) & (uint64_t)mask;
            any = true;
          }
        }
    }
#pragma unroll
    for (int q = 0; q < PW_HT_PROBE_Q; ++q) {
      const int64_t j = i + q * stride;
      if (j < nq) {
        out[j] = v[q];
        found[j] = v[q] != -1;
      }
    }
  }
}

extern "C" int pw_ht_build(const void* klo, const void* khi, const void* vals,
                           int64_t m, void* tab, int64_t nslots,
                           void* stream) {
  hipStream_t s = (hipStream_t)stream;
  int64_t nblocks = (m + PW_BLOCK - 1) / PW_BLOCK;
  if (nblocks > 4096) nblocks = 4096;
  if (nblocks < 1) nblocks = 1;
  hipLaunchKernelGGL(k_ht_build, dim3((uint32_t)nblocks), dim3(PW_BLOCK), 0, s,
                     (const int64_t*)klo, (const int64_t*)khi,
                     (const int64_t*)vals, m, PwHt{(long long*)tab},
                     nslots - 1);
  return (int)hipGetLastError();
}

extern "C" int pw_ht_probe(const void* qlo, const void* qhi, int64_t nq,
                           const void* tab, int64_t nslots, void* out,
                           void* found, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  const int64_t per_block = (int64_t)PW_BLOCK * PW_HT_PROBE_Q;
  int64_t nblocks = (nq + per_block - 1) / per_block;
  if (nblocks > 4096) nblocks = 4096;
  if (nblocks < 1) nblocks = 1;
  hipLaunchKernelGGL(k_ht_probe, dim3((uint32_t)nblocks), dim3(PW_BLOCK), 0, s,
                     (const int64_t*)qlo, (const int64_t*)qhi, nq,
                     PwHt{(long long*)tab}, nslots - 1, (int64_t*)out,
                     (bool*)found);
  return (int)hipGetLastError();
}

// ------------------------------------------------- hash table: intern --
// Insert-or-get on the same table (same slots, -1 still empty):
// known keys return their stored code, the batch's distinct new keys get
// codes base, base+1, ... in order of first occurrence by row index —
// what StringPool.codes() assigns on the host.  Four launches, lock-free,
// no lane ever waits on a value another lane is expected to write:
//
//   claim    row i linear-probes.  A slot with val >= 0 is compared by
//            its key words (written by an earlier launch).  A slot with
//            val <= -2 is pending: it encodes its claimer row r as -(r+2)
//            and is compared against qlo[r]/qhi[r] — the batch is
//            immutable, so a pending slot's key words are never read.
//            Equal keys atomicMax the slot so the smallest row wins; an
//            empty slot is claimed by CAS, and a lost CAS re-examines the
//            same slot with the value the CAS returned.  A slot's key
//            identity is fixed once claimed and slots are never emptied,
//            so a key cannot land in two slots.  Hits store their code;
//            pending rows store their slot and set pend[i] = 1.
//            Plain val loads may be stale within the launch; that is
//            harmless: a stale -1 is corrected by the CAS's return value,
//            a stale pending value names another row with the same key,
//            and no value >= 0 is written during the launch.
//   count    pending row i is a winner iff the slot's val == -(i+2); mark
//            pend[i] = 2 and count winners per block chunk.
//   commit   every block sums the counts of the chunks before it, then
//            ranks its winners in row order; winner k writes the
//            slot's key, the dictionary hash arrays at base+k,
//            first_row[k] = i and, last, the slot's val = base+k.
//   resolve  the other pending rows read their slot's now-final code.
//
// On the all-known path count/commit/resolve only stream the n pend
// bytes.  Probing stops after nslots probes and raises err[0] (the caller
// keeps the load factor <= 0.5, so this never triggers in a sound run).
//
// Optional front table: the probe bound forces the caller to size the
// table above for a batch of nothing but new keys, far past the caches
// for a large batch.  A caller may keep the keys it knows for certain in
// a second, compact table of the same layout ("front", read-only here):
// claim probes it first as k_ht_probe does (pw_ht_find) and only its misses
// touch the open table.  A key is in at most one of the two.

#define PW_HT_ERR_PROBE 1     // table full / probe bound hit
#define PW_HT_ERR_STATE 2     // slot or claimer row out of range
#define PW_HT_ERR_CAPACITY 4  // dictionary arrays or byte arena too small

__global__ void k_ht_intern_claim(const int64_t* __restrict__ qlo,
                                  const int64_t* __restrict__ qhi, int64_t n,
                                  const PwHt tab, int64_t nslots,
                                  const PwHt front, int64_t front_nslots,
                                  int64_t* __restrict__ codes,
                                  uint8_t* __restrict__ pend, long long* err) {
  const uint64_t mask = (uint64_t)(nslots - 1);
  const uint64_t fmask = (uint64_t)(front_nslots - 1);
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) {
    const int64_t lo = qlo[i], hi = qhi[i];
    if (front_nslots) {
      const long long fv = pw_ht_find(front, fmask, lo, hi, front_nslots);
      if (fv >= 0) {
        codes[i] = (int64_t)fv;
        pend[i] = 0;
        continue;
      }
    }
    const long long me = -(long long)(i + 2);
    uint64_t slot = (uint64_t)lo & mask;
    int64_t out = -1;
    uint8_t p = 0;
    int e = PW_HT_ERR_PROBE;
    long long tv = *tab.val(slot);
    for (int64_t probes = 0; probes < nslots; ++probes) {
      if (tv == -1) {
        tv = (long long)atomicCAS((unsigned long long*)tab.val(slot),
                                  (unsigned long long)(long long)-1,
                                  (unsigned long long)me);
        if (tv == -1) {  // claimed
          out = (int64_t)slot, p = 1, e = 0;
          break;
        }
      }
      if (tv >= 0) {
        const PwHtKey k = tab.key(slot);
        if (k.lo == lo && k.hi == hi) {
          out = (int64_t)tv, e = 0;
          break;
        }
      } else {
        const int64_t r = -(tv + 2);
        if (r < 0 || r >= n) {
          e = PW_HT_ERR_STATE;
          break;
        }
        if (qlo[r] == lo && qhi[r] == hi) {
          if (me > tv)
            __hip_atomic_fetch_max(tab.val(slot), me, __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
          out = (int64_t)slot, p = 1, e = 0;
          break;
        }
      }
      slot = (slot + 1) & mask;
      tv = *tab.val(slot);
    }
    if (e) atomicOr((unsigned long long*)err, (unsigned long long)e);
    codes[i] = out;
    pend[i] = p;
  }
}

// rows [start, end) of one block, 16 rows (one pend granule) per lane
__global__ void k_ht_intern_count(int64_t n, int64_t chunk,
                                  const int64_t* __restrict__ codes,
                                  uint8_t* pend, const PwHt tab,
                                  int64_t nslots, long long* block_counts,
                                  long long* err) {
  __shared__ int cnt;
  if (threadIdx.x == 0) cnt = 0;
  __syncthreads();
  int64_t start = (int64_t)blockIdx.x * chunk;
  int64_t end = min(start + chunk, n);
  int local = 0;
  for (int64_t tile = start; tile < end; tile += (int64_t)blockDim.x * 16) {
    int64_t g = tile + (int64_t)threadIdx.x * 16;
    if (g >= end) continue;
    if (g + 16 <= end) {  // chunk and pend base are 16B-aligned
      uint4 v = *(const uint4*)(pend + g);
      if ((v.x | v.y | v.z | v.w) == 0) continue;
    }
    for (int64_t i = g; i < min(g + 16, end); ++i) {
      if (!pend[i]) continue;
      int64_t slot = codes[i];
      if (slot < 0 || slot >= nslots) {
        atomicOr((unsigned long long*)err, (unsigned long long)PW_HT_ERR_STATE);
        pend[i] = 0;
        continue;
      }
      if (*tab.val((uint64_t)slot) == -(long long)(i + 2)) {
        pend[i] = 2;
        ++local;
      }
    }
  }
  if (local) atomicAdd(&cnt, local);
  __syncthreads();
  if (threadIdx.x == 0) block_counts[blockIdx.x] = cnt;
}

__global__ void k_ht_intern_commit(
    const int64_t* __restrict__ qlo, const int64_t* __restrict__ qhi,
    int64_t n, int64_t chunk, int64_t* codes, const uint8_t* __restrict__ pend,
    const long long* __restrict__ block_counts,
    const long long* __restrict__ base_ptr, const PwHt tab, int64_t* pool_lo,
    int64_t* pool_hi, int64_t pool_cap,
    int64_t* first_row, long long* n_new, long long* err) {
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  __shared__ unsigned long long cursor;
  __shared__ int wave_tot[PW_BLOCK / 64];
  // this block's first rank: the winners of the blocks before it (at most
  // 2048 counts, so every block sums them itself — no scan launch)
  if (threadIdx.x == 0) cursor = 0;
  __syncthreads();
  unsigned long long part = 0;
  for (int j = threadIdx.x; j < (int)blockIdx.x; j += blockDim.x)
    part += (unsigned long long)block_counts[j];
  if (part) atomicAdd(&cursor, part);
  __syncthreads();
  if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0)
    n_new[0] = (long long)cursor + block_counts[blockIdx.x];
  const long long base = base_ptr[0];
  int64_t start = (int64_t)blockIdx.x * chunk;
  int64_t end = min(start + chunk, n);
  for (int64_t tile = start; tile < end; tile += (int64_t)blockDim.x * 16) {
    int64_t g = tile + (int64_t)threadIdx.x * 16;
    unsigned wmask = 0;
    if (g < end) {
      bool any = true;
      if (g + 16 <= end) {
        uint4 v = *(const uint4*)(pend + g);
        any = (v.x | v.y | v.z | v.w) != 0;
      }
      if (any)
        for (int j = 0; j < 16 && g + j < end; ++j)
          if (pend[g + j] == 2) wmask |= 1u << j;
    }
    int hits = __popc(wmask);
    int incl = hits;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      int v = __shfl_up(incl, off, 64);
      if (lane >= off) incl += v;
    }
    if (lane == 63) wave_tot[wave] = incl;
    __syncthreads();
    int wbase = 0;
    for (int w = 0; w < wave; ++w) wbase += wave_tot[w];
    long long k = (long long)cursor + wbase + (incl - hits);
    while (wmask) {
      int j = __ffs(wmask) - 1;
      wmask &= wmask - 1;
      const int64_t i = g + j;
      const int64_t slot = codes[i];  // range-checked by k_ht_intern_count
      const long long code = base + k;
      if (code < 0 || code >= pool_cap) {
        atomicOr((unsigned long long*)err,
                 (unsigned long long)PW_HT_ERR_CAPACITY);
      } else {
        const int64_t lo = qlo[i], hi = qhi[i];
        tab.set_key((uint64_t)slot, lo, hi);
        pool_lo[code] = lo;
        pool_hi[code] = hi;
        first_row[k] = i;  // k < winners <= n
        *tab.val((uint64_t)slot) = code;
        codes[i] = code;
      }
      ++k;
    }
    __syncthreads();
    if (threadIdx.x == (int)blockDim.x - 1) cursor += wbase + incl;
    __syncthreads();
  }
}

__global__ void k_ht_intern_resolve(int64_t n, int64_t chunk, int64_t* codes,
                                    const uint8_t* __restrict__ pend,
                                    const PwHt tab) {
  int64_t start = (int64_t)blockIdx.x * chunk;
  int64_t end = min(start + chunk, n);
  for (int64_t tile = start; tile < end; tile += (int64_t)blockDim.x * 16) {
    int64_t g = tile + (int64_t)threadIdx.x * 16;
    if (g >= end) continue;
    if (g + 16 <= end) {
      uint4 v = *(const uint4*)(pend + g);
      if ((v.x | v.y | v.z | v.w) == 0) continue;
    }
    for (int64_t i = g; i < min(g + 16, end); ++i) {
      if (pend[i] != 1) continue;
      long long tv = *tab.val((uint64_t)codes[i]);
      codes[i] = tv >= 0 ? (int64_t)tv : -1;  // < 0 only after a flagged error
    }
  }
}

static inline int64_t pw_intern_chunk(int64_t n, int64_t nblocks) {
  int64_t chunk = ((n + nblocks - 1) / nblocks + 15) & ~(int64_t)15;
  return chunk < 16 ? 16 : chunk;
}

// One call enqueues the four launches.  nblocks (<= 2048) is the number
// of row chunks of count/commit/resolve; block_counts has nblocks entries,
// n_new one.
extern "C" int pw_ht_intern(const void* qlo, const void* qhi, int64_t n,
                            void* tab, int64_t nslots, const void* front,
                            int64_t front_nslots, const void* base_ptr,
                            void* pool_lo, void* pool_hi, int64_t pool_cap,
                            void* codes, void* pend, void* first_row,
                            void* block_counts, int64_t nblocks, void* n_new,
                            void* err, void* stream) {
  if (n <= 0 || nblocks < 1 || nblocks > 2048) return -2;
  if (nslots < 1 || (nslots & (nslots - 1))) return -2;
  if (front_nslots < 0 || (front_nslots & (front_nslots - 1))) return -2;
  hipStream_t s = (hipStream_t)stream;
  int64_t cblocks = (n + PW_BLOCK - 1) / PW_BLOCK;
  if (cblocks > 4096) cblocks = 4096;
  int64_t chunk = pw_intern_chunk(n, nblocks);
  const PwHt t{(long long*)tab};
  const PwHt f{(long long*)const_cast<void*>(front)};  // only read
  hipLaunchKernelGGL(k_ht_intern_claim, dim3((uint32_t)cblocks),
                     dim3(PW_BLOCK), 0, s, (const int64_t*)qlo,
                     (const int64_t*)qhi, n, t, nslots, f, front_nslots,
                     (int64_t*)codes, (uint8_t*)pend, (long long*)err);
  hipLaunchKernelGGL(k_ht_intern_count, dim3((uint32_t)nblocks),
                     dim3(PW_BLOCK), 0, s, n, chunk, (const int64_t*)codes,
                     (uint8_t*)pend, t, nslots, (long long*)block_counts,
                     (long long*)err);
  hipLaunchKernelGGL(k_ht_intern_commit, dim3((uint32_t)nblocks),
                     dim3(PW_BLOCK), 0, s, (const int64_t*)qlo,
                     (const int64_t*)qhi, n, chunk, (int64_t*)codes,
                     (const uint8_t*)pend, (const long long*)block_counts,
                     (const long long*)base_ptr, t, (int64_t*)pool_lo,
                     (int64_t*)pool_hi, pool_cap, (int64_t*)first_row,
                     (long long*)n_new, (long long*)err);
  hipLaunchKernelGGL(k_ht_intern_resolve, dim3((uint32_t)nblocks),
                     dim3(PW_BLOCK), 0, s, n, chunk, (int64_t*)codes,
                     (const uint8_t*)pend, t);
  return (int)hipGetLastError();
}

// Pack the byte spans of the batch's new tokens into the dictionary's
// arena.  Token k (k < *n_new) is row first_row[k]; its bytes go to a
// range reserved with one cursor atomicAdd per wave (wave scan of the
// lengths), and (offset, length) are recorded at code base+k, so the
// arena layout may vary run to run while the decoded strings do not.
__global__ void k_gather_spans(const uint8_t* __restrict__ buf, int64_t nbuf,
                               const int64_t* __restrict__ starts,
                               const int64_t* __restrict__ ends, int64_t nrows,
                               const int64_t* __restrict__ first_row,
                               const long long* __restrict__ n_new_ptr,
                               const long long* __restrict__ base_ptr,
                               uint8_t* arena, int64_t arena_cap,
                               unsigned long long* cursor, int64_t* tok_off,
                               int64_t* tok_len, int64_t pool_cap,
                               long long* err) {
  const int lane = threadIdx.x & 63;
  long long n_new = n_new_ptr[0];
  if (n_new > nrows) n_new = nrows;
  const long long base = base_ptr[0];
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  // whole waves iterate together (the bound is rounded up per wave)
  const int64_t k0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (int64_t k = k0; k - lane < n_new; k += stride) {
    int64_t s = 0, len = 0;
    bool ok = k < n_new && base + k >= 0 && base + k < pool_cap;
    if (ok) {
      int64_t row = first_row[k];
      ok = row >= 0 && row < nrows;
      if (ok) {
        s = starts[row];
        int64_t e = ends[row];
        ok = s >= 0 && e >= s && e <= nbuf;
        len = ok ? e - s : 0;
      }
    }
    if (k < n_new && !ok)
      atomicOr((unsigned long long*)err,
               (unsigned long long)(base + k < pool_cap ? PW_HT_ERR_STATE
                                                        : PW_HT_ERR_CAPACITY));
    long long incl = len;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      long long v = __shfl_up(incl, off, 64);
      if (lane >= off) incl += v;
    }
    long long total = __shfl(incl, 63, 64);
    unsigned long long wbase = 0;
    if (lane == 0 && total) wbase = atomicAdd(cursor, (unsigned long long)total);
    wbase = __shfl(wbase, 0, 64);
    if (!ok) continue;
    int64_t off = (int64_t)wbase + (incl - len);
    if (off + len > arena_cap) {
      atomicOr((unsigned long long*)err,
               (unsigned long long)PW_HT_ERR_CAPACITY);
      off = 0, len = 0;
    }
    for (int64_t b = 0; b < len; ++b) arena[off + b] = buf[s + b];
    tok_off[base + k] = off;
    tok_len[base + k] = len;
  }
}

extern "C" int pw_gather_spans(const void* buf, int64_t nbuf,
                               const void* starts, const void* ends,
                               int64_t nrows, const void* first_row,
                               const void* n_new_ptr, const void* base_ptr,
                               void* arena, int64_t arena_cap, void* cursor,
                               void* tok_off, void* tok_len, int64_t pool_cap,
                               void* err, void* stream) {
  if (nrows <= 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(k_gather_spans, dim3(pw_grid(nrows) > 256 ? 256 : pw_grid(nrows)),
                     dim3(PW_BLOCK), 0, s, (const uint8_t*)buf, nbuf,
                     (const int64_t*)starts, (const int64_t*)ends, nrows,
                     (const int64_t*)first_row, (const long long*)n_new_ptr,
                     (const long long*)base_ptr, (uint8_t*)arena, arena_cap,
                     (unsigned long long*)cursor, (int64_t*)tok_off,
                     (int64_t*)tok_len, pool_cap, (long long*)err);
  return (int)hipGetLastError();
}

extern "C" int pw_gather_cols(const void* idx, int64_t m, int ncols,
                              void* const* srcs, void* const* dsts,
                              void* stream) {
  if (ncols < 1 || ncols > 8) return -2;
  hipStream_t s = (hipStream_t)stream;
  PwGather8 p;
  for (int c = 0; c < ncols; ++c) {
    p.src[c] = (const long long*)srcs[c];
    p.dst[c] = (long long*)dsts[c];
  }
  int64_t nblocks = (m + PW_BLOCK - 1) / PW_BLOCK;
  if (nblocks > 4096) nblocks = 4096;
  if (nblocks < 1) nblocks = 1;
  hipLaunchKernelGGL(k_gather_cols, dim3((uint32_t)nblocks), dim3(PW_BLOCK),
                     0, s, (const long long*)idx, m, ncols, p);
  return (int)hipGetLastError();
}

// ------------------------------------------------------- group combine --
// The groupby combiner on interleaved (n,2) int64 keys, start to finish:
// rows of (key128, contributions...) -> (unique key, sums, first row).
//
//   sort     rocprim::radix_sort_pairs over word0, read in place from the
//            16-byte rows through a transform iterator; the payload is a
//            32-bit row index from a counting iterator (12 B/row per
//            onesweep pass instead of torch.sort's 16, no arange, no
//            de-stacked key copy)
//   gather   k_gc_gather_k1: word1 through the permutation, once
//   repair   k_gc_sort_repair: k_sort_repair on a uint32 permutation
//   count    k_segred_count, as is
//   emit     k_gc_emit: k_segred_emit reading the contributions THROUGH
//            the permutation (no sorted contribution column is written)
//            and emitting the original row id of each segment start
//
// The sort is stable and the repair swaps only strictly out-of-order
// word1 pairs, so equal keys keep ascending row order and a segment's
// first row is its smallest row index.  Signed int64 key order (rocPRIM
// flips the sign bit for signed key types), matching the state's order.
//
// This is the full 64-bit sort.  The default is the prefix sort further
// down; this one is its fallback and the PW_GC_FULL_SORT=1 comparison path.

struct GcWord0 {
  const long long* keys;  // (n,2) row-major
  __host__ __device__ long long operator()(uint32_t i) const {
    return keys[2 * (size_t)i];
  }
};

using GcKeyIter =
    rocprim::transform_iterator<rocprim::counting_iterator<uint32_t>, GcWord0,
                                long long>;

static hipError_t gc_sort(void* temp, size_t& temp_bytes, const long long* keys,
                          long long* k0_sorted, uint32_t* perm32, int64_t n,
                          hipStream_t s) {
  GcKeyIter kin(rocprim::counting_iterator<uint32_t>(0), GcWord0{keys});
  rocprim::counting_iterator<uint32_t> vin(0);
  return rocprim::radix_sort_pairs(temp, temp_bytes, kin, k0_sorted, vin,
                                   perm32, (size_t)n, 0, 64, s);
}

// ctrl: the two control words of k_gc_mark_dirty (below), cleared here
__global__ void k_gc_gather_k1(const long long* __restrict__ keys,
                               const uint32_t* __restrict__ perm32,
                               long long* __restrict__ k1_sorted, int64_t n,
                               unsigned long long* ctrl) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  if (i == 0) {
    ctrl[0] = 0;
    ctrl[1] = 0;
  }
  for (; i < n; i += stride) k1_sorted[i] = keys[2 * (size_t)perm32[i] + 1];
}

__global__ void k_gc_sort_repair(const long long* __restrict__ k0,
                                 long long* k1, uint32_t* perm32, int64_t n,
                                 int parity) {
  int64_t i = 2 * ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) + parity;
  if (i + 1 >= n) return;
  if (k0[i] != k0[i + 1]) return;
  long long a = k1[i], b = k1[i + 1];
  if (a > b) {
    k1[i] = b;
    k1[i + 1] = a;
    uint32_t p = perm32[i];
    perm32[i] = perm32[i + 1];
    perm32[i + 1] = p;
  }
}

// block_csum is the INCLUSIVE prefix sum of k_segred_count's block counts.
// POS (the mixed combiner, pw_gc_emit_pos) also writes every segment's start
// position in sorted order to out_pos, and n to out_pos[nseg]; the int-only
// instantiation compiles to the kernel it was before the flag.
template <bool POS>
__global__ void k_gc_emit(const long long* __restrict__ k0,
                          const long long* __restrict__ k1,
                          const uint32_t* __restrict__ perm32,
                          AccPtrs contribs, int nacc, int64_t n,
                          const long long* __restrict__ block_csum,
                          long long* out_k0, long long* out_k1,
                          long long* out_first, AccPtrsMut out_accs,
                          long long* out_pos) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int lane = threadIdx.x & 63;
  int flag = 0;
  long long a0 = 0, a1 = 0;
  uint32_t row = 0;
  if (i < n) {
    a0 = k0[i];
    a1 = k1[i];
    row = perm32[i];
    flag = (i == 0) || a0 != k0[i - 1] || a1 != k1[i - 1];
  }
  // block-wide exclusive scan of flags via per-wave ballot + LDS
  uint64_t ball = __ballot(flag);
  int wave = threadIdx.x >> 6;
  __shared__ int wave_tot[PW_BLOCK / 64];
  if (lane == 0) wave_tot[wave] = __popcll(ball);
  __syncthreads();
  int wave_base = 0;
  for (int j = 0; j < wave; ++j) wave_base += wave_tot[j];
  uint64_t below = ball & ((lane == 0) ? 0ULL : ((1ULL << lane) - 1));
  int local_excl = wave_base + __popcll(below);
  long long base = blockIdx.x ? block_csum[blockIdx.x - 1] : 0;
  long long sid = base + local_excl + flag - 1;
  if (i < n && flag) {
    out_k0[sid] = a0;
    out_k1[sid] = a1;
    out_first[sid] = (long long)row;
    if (POS) out_pos[sid] = i;
  }
  if (POS && i == n - 1) out_pos[block_csum[gridDim.x - 1]] = n;
  // wave-segmented sums per accumulator; padding lanes carry the sentinel
  // -1 so a real row followed by padding still detects its run tail
  long long s = (i < n) ? sid : -1;
  long long nxt = __shfl_down(s, 1, 64);
  bool tail = (lane == 63) || (nxt != s);
  for (int a = 0; a < nacc; ++a) {
    long long v = (i < n) ? contribs.p[a][row] : 0;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      long long vv = __shfl_up(v, off, 64);
      long long ss = __shfl_up(s, off, 64);
      if (lane >= off && ss == s) v += vv;
    }
    if (s >= 0 && tail)
      atomicAdd((unsigned long long*)&out_accs.p[a][s],
                (unsigned long long)v);
  }
}

// bytes of rocPRIM temp storage the sort needs for n rows (0 on error)
extern "C" int64_t pw_gc_temp_bytes(int64_t n) {
  size_t bytes = 0;
  if (n <= 0 || n >= ((int64_t)1 << 32)) return 0;
  if (gc_sort(nullptr, bytes, nullptr, nullptr, nullptr, n, 0) != hipSuccess)
    return 0;
  return (int64_t)bytes;
}

// ------------------------------------------- group combine, prefix sort --
// word0 is a 64-bit hash, so its top 32 bits already separate all but a
// handful of keys.  The default path sorts only that prefix and mends the
// few rows that tie on it:
//
//   sort     rocprim::radix_sort_pairs on a uint32 key (top prefix_bits of
//            word0, see GcPrefix) with the uint32 row payload: four
//            8-bit passes at 8 B/row instead of eight at 12 B/row.  The
//            sorted keys are scratch.
//   gather   k_gc_gather_k01: word0 and word1 through the permutation
//   mark     k_gc_mark_dirty: lists the start of every prefix run that
//            holds more than one distinct key; writes none of the arrays
//   repair   k_gc_repair_runs: one block per listed run, stable rank sort
//            of (word0, word1) in LDS, written back in place
//   count, emit   as above
//
// After the repair k0_sorted, k1_sorted and perm32 are what the 64-bit
// sort above produces: the prefix sort is stable with an ascending
// payload, and the rank is stable, so equal keys keep ascending row order.
// A run longer than max_run, or more than max_dirty runs, raises the
// overflow word instead; the caller then redoes the batch with
// pw_gc_sort_count.  ctrl[0] is that overflow word, ctrl[1] the number of
// listed runs; the gather kernel clears both, so no memset is queued.

#define PW_GC_REPAIR_GRID 64
#define PW_GC_MAX_RUN_LIMIT 3072  // 20 B/row of LDS: 60 KB

// The sort key: the top prefix_bits of word0 with the sign bit flipped
// (unsigned order = signed int64 order), moved down to bit 0, so the sort
// runs on bits [0, prefix_bits).  Sorting bits [32 - prefix_bits, 32) of
// the unshifted word is the same order, but below its onesweep threshold
// rocPRIM's merge path builds that range's mask with a 32-bit shift by 32
// and then compares the wrong bits.
struct GcPrefix {
  const long long* keys;  // (n,2) row-major
  int drop;               // 32 - prefix_bits
  __host__ __device__ uint32_t operator()(uint32_t i) const {
    uint32_t top = (uint32_t)((uint64_t)keys[2 * (size_t)i] >> 32);
    return (top ^ 0x80000000u) >> drop;
  }
};

using GcPrefixIter =
    rocprim::transform_iterator<rocprim::counting_iterator<uint32_t>, GcPrefix,
                                uint32_t>;

static hipError_t gc_sort_prefix(void* temp, size_t& temp_bytes,
                                 const long long* keys, uint32_t* prefix_sorted,
                                 uint32_t* perm32, int64_t n, int prefix_bits,
                                 hipStream_t s) {
  GcPrefixIter kin(rocprim::counting_iterator<uint32_t>(0),
                   GcPrefix{keys, 32 - prefix_bits});
  rocprim::counting_iterator<uint32_t> vin(0);
  return rocprim::radix_sort_pairs(temp, temp_bytes, kin, prefix_sorted, vin,
                                   perm32, (size_t)n, 0u,
                                   (unsigned int)prefix_bits, s);
}

__global__ void k_gc_gather_k01(const long long* __restrict__ keys,
                                const uint32_t* __restrict__ perm32,
                                long long* __restrict__ k0_sorted,
                                long long* __restrict__ k1_sorted, int64_t n,
                                unsigned long long* ctrl) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  if (i == 0) {
    ctrl[0] = 0;
    ctrl[1] = 0;
  }
  for (; i < n; i += stride) {
    size_t r = 2 * (size_t)perm32[i];
    k0_sorted[i] = keys[r];
    k1_sorted[i] = keys[r + 1];
  }
}

__global__ void k_gc_mark_dirty(const long long* __restrict__ k0,
                                const long long* __restrict__ k1, int64_t n,
                                int shift, uint32_t max_run,
                                uint32_t max_dirty, uint32_t* dirty_list,
                                unsigned long long* ctrl) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < 1 || i >= n) return;
  long long c0 = k0[i], p0 = k0[i - 1];
  uint64_t pref = (uint64_t)c0 >> shift;
  if (((uint64_t)p0 >> shift) != pref) return;
  long long p1 = k1[i - 1];
  if (c0 == p0 && k1[i] == p1) return;
  // row i is a dirty boundary.  Rows left of it equal row i-1 until the
  // run start or an earlier dirty boundary; only the first boundary of a
  // run lists the run.
  int64_t j = i - 1;
  uint32_t steps = 0;
  while (j > 0) {
    long long q0 = k0[j - 1];
    if (((uint64_t)q0 >> shift) != pref) break;       // j starts the run
    if (q0 != p0 || k1[j - 1] != p1) return;          // j is a boundary
    --j;
    if (++steps > max_run) {
      ctrl[0] = 1;
      return;
    }
  }
  unsigned long long slot = atomicAdd(&ctrl[1], 1ULL);
  if (slot < max_dirty) dirty_list[slot] = (uint32_t)j;
  else ctrl[0] = 1;
}

__global__ void k_gc_repair_runs(long long* k0, long long* k1,
                                 uint32_t* perm32, int64_t n, int shift,
                                 uint32_t max_run, uint32_t max_dirty,
                                 const uint32_t* __restrict__ dirty_list,
                                 unsigned long long* ctrl) {
  extern __shared__ long long gc_lds[];
  long long* s0 = gc_lds;
  long long* s1 = gc_lds + max_run;
  uint32_t* sp = (uint32_t*)(gc_lds + 2 * (size_t)max_run);
  __shared__ uint32_t run_len;
  unsigned long long listed = ctrl[1];
  uint32_t cnt = listed < max_dirty ? (uint32_t)listed : max_dirty;
  for (uint32_t e = blockIdx.x; e < cnt; e += gridDim.x) {
    int64_t s = dirty_list[e];
    uint64_t pref = (uint64_t)k0[s] >> shift;
    if (threadIdx.x == 0) run_len = max_run + 1;
    __syncthreads();
    // first row right of s, at most max_run away, that leaves the run
    for (uint32_t r = 1 + threadIdx.x; r <= max_run; r += blockDim.x) {
      int64_t idx = s + r;
      if (idx >= n || ((uint64_t)k0[idx] >> shift) != pref) {
        atomicMin(&run_len, r);
        break;
      }
    }
    __syncthreads();
    uint32_t len = run_len;
    if (len > max_run) {
      if (threadIdx.x == 0) ctrl[0] = 1;
    } else {
      for (uint32_t t = threadIdx.x; t < len; t += blockDim.x) {
        s0[t] = k0[s + t];
        s1[t] = k1[s + t];
        sp[t] = perm32[s + t];
      }
      __syncthreads();
      for (uint32_t t = threadIdx.x; t < len; t += blockDim.x) {
        long long a0 = s0[t], a1 = s1[t];
        uint32_t rank = 0;
        for (uint32_t u = 0; u < len; ++u) {
          long long b0 = s0[u], b1 = s1[u];
          bool before = b0 < a0 ||
                        (b0 == a0 && (b1 < a1 || (b1 == a1 && u < t)));
          rank += before ? 1u : 0u;
        }
        k0[s + rank] = a0;
        k1[s + rank] = a1;
        perm32[s + rank] = sp[t];
      }
    }
    __syncthreads();
  }
}

// mark + repair + segment count on gathered (k0, k1, perm32)
static int gc_repair_count(void* k0_sorted, void* k1_sorted, void* perm32,
                           int64_t n, int shift, int64_t max_run,
                           int64_t max_dirty, void* dirty_list, void* ctrl,
                           void* block_counts, hipStream_t s) {
  int64_t nblocks = (n + PW_BLOCK - 1) / PW_BLOCK;
  hipLaunchKernelGGL(k_gc_mark_dirty, dim3((uint32_t)nblocks), dim3(PW_BLOCK),
                     0, s, (const long long*)k0_sorted,
                     (const long long*)k1_sorted, n, shift, (uint32_t)max_run,
                     (uint32_t)max_dirty, (uint32_t*)dirty_list,
                     (unsigned long long*)ctrl);
  size_t lds = (size_t)max_run * 20;
  hipLaunchKernelGGL(k_gc_repair_runs, dim3(PW_GC_REPAIR_GRID),
                     dim3(PW_BLOCK), lds, s, (long long*)k0_sorted,
                     (long long*)k1_sorted, (uint32_t*)perm32, n, shift,
                     (uint32_t)max_run, (uint32_t)max_dirty,
                     (const uint32_t*)dirty_list, (unsigned long long*)ctrl);
  SegWords w;
  w.p[0] = (const int64_t*)k0_sorted;
  w.p[1] = (const int64_t*)k1_sorted;
  hipLaunchKernelGGL(k_segred_count, dim3((uint32_t)nblocks), dim3(PW_BLOCK),
                     0, s, w, 2, n, (int*)block_counts);
  return (int)hipGetLastError();
}

// 64-bit sort + word1 gather + repair + segment count, all on the caller's
// stream.  keys: (n,2) int64 rows 16 B apart.  Outputs: k0_sorted,
// k1_sorted (n int64), perm32 (n uint32), block_counts (ceil(n/256) int32),
// dirty_list and ctrl as in pw_gc_prefix_sort_count.  The odd-even passes
// put right equal-word0 runs of up to passes+1 rows with distinct keys;
// mark + repair on the whole of word0 (shift 0) then sort what they cannot:
// longer runs and runs with repeated keys.  Overflow is left to the caller.
extern "C" int pw_gc_sort_count(const void* keys, int64_t n, void* temp,
                                int64_t temp_bytes, void* k0_sorted,
                                void* k1_sorted, void* perm32, int passes,
                                int64_t max_run, int64_t max_dirty,
                                void* dirty_list, void* ctrl,
                                void* block_counts, void* stream) {
  if (n < 2 || n >= ((int64_t)1 << 32)) return 1;
  if (max_run < 2 || max_run > PW_GC_MAX_RUN_LIMIT) return 1;
  if (max_dirty < 1 || max_dirty >= ((int64_t)1 << 32)) return 1;
  hipStream_t s = (hipStream_t)stream;
  size_t tb = (size_t)temp_bytes;
  hipError_t e = gc_sort(temp, tb, (const long long*)keys,
                         (long long*)k0_sorted, (uint32_t*)perm32, n, s);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(k_gc_gather_k1, dim3(2 * PW_MAX_GRID), dim3(PW_BLOCK), 0,
                     s, (const long long*)keys, (const uint32_t*)perm32,
                     (long long*)k1_sorted, n, (unsigned long long*)ctrl);
  int64_t pairs = n / 2 + 1;
  int64_t rblocks = (pairs + PW_BLOCK - 1) / PW_BLOCK;
  for (int p = 0; p < passes; ++p)
    hipLaunchKernelGGL(k_gc_sort_repair, dim3((uint32_t)rblocks),
                       dim3(PW_BLOCK), 0, s, (const long long*)k0_sorted,
                       (long long*)k1_sorted, (uint32_t*)perm32, n, p & 1);
  return gc_repair_count(k0_sorted, k1_sorted, perm32, n, 0, max_run,
                         max_dirty, dirty_list, ctrl, block_counts, s);
}

extern "C" int64_t pw_gc_temp_bytes_prefix(int64_t n) {
  size_t bytes = 0;
  if (n <= 0 || n >= ((int64_t)1 << 32)) return 0;
  if (gc_sort_prefix(nullptr, bytes, nullptr, nullptr, nullptr, n, 32, 0) !=
      hipSuccess)
    return 0;
  return (int64_t)bytes;
}

// prefix sort + gather + mark + repair + segment count, all on the caller's
// stream.  Outputs as pw_gc_sort_count, plus dirty_list (max_dirty uint32)
// and ctrl (2 uint64: overflow, listed runs).  k1_sorted doubles as the
// scratch for the sorted prefixes until the gather overwrites it.
extern "C" int pw_gc_prefix_sort_count(const void* keys, int64_t n, void* temp,
                                       int64_t temp_bytes, void* k0_sorted,
                                       void* k1_sorted, void* perm32,
                                       int prefix_bits, int64_t max_run,
                                       int64_t max_dirty, void* dirty_list,
                                       void* ctrl, void* block_counts,
                                       void* stream) {
  if (n < 2 || n >= ((int64_t)1 << 32)) return 1;
  if (prefix_bits < 1 || prefix_bits > 32) return 1;
  if (max_run < 2 || max_run > PW_GC_MAX_RUN_LIMIT) return 1;
  if (max_dirty < 1 || max_dirty >= ((int64_t)1 << 32)) return 1;
  hipStream_t s = (hipStream_t)stream;
  size_t tb = (size_t)temp_bytes;
  hipError_t e = gc_sort_prefix(temp, tb, (const long long*)keys,
                                (uint32_t*)k1_sorted, (uint32_t*)perm32, n,
                                prefix_bits, s);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(k_gc_gather_k01, dim3(2 * PW_MAX_GRID), dim3(PW_BLOCK), 0,
                     s, (const long long*)keys, (const uint32_t*)perm32,
                     (long long*)k0_sorted, (long long*)k1_sorted, n,
                     (unsigned long long*)ctrl);
  return gc_repair_count(k0_sorted, k1_sorted, perm32, n, 64 - prefix_bits,
                         max_run, max_dirty, dirty_list, ctrl, block_counts,
                         s);
}

// ------------------------------------------ group combine, bucket path --
// The result needs the distinct keys in order and a sum per key, not the
// order of all n rows.  This path orders the rows only as far as a bucket
// (the top bucket_bits of word0: one radix pass) and aggregates each bucket
// in LDS:
//
//   partition  bucket_bits <= 8 (the partition layout): the rows themselves
//              are moved into bucket order, read once in row order.
//                k_gc_part_count    per-workgroup LDS histogram of a fixed
//                                   tile of rows, block_hist[block][bucket]
//                k_gc_part_scan     one workgroup: bucket totals to
//                                   bucket_start[0..nb], and the first output
//                                   position per bucket of each of 32 ranges
//                                   of workgroups; clears ctl[0..1]
//                k_gc_part_scatter  the same tile again (16-B key, row index
//                                   and every contribution): part_keys (n,2),
//                                   part_row, part_acc[a], grouped by bucket;
//                                   its own first positions are its range's
//                                   plus the counts of the blocks before it
//              The order of the rows inside a bucket is whatever the LDS
//              cursors hand out: sums are unsigned adds and the first row is
//              a min, so the result does not depend on it.  No sort, no
//              memset, no temp storage.
//              bucket_bits > 8 or the gather layout: gc_sort_prefix with
//              prefix_bits = bucket_bits (perm32 grouped by bucket, rows
//              ascending inside a bucket), then k_gc_bucket_bounds: the
//              2^bucket_bits + 1 bucket offsets by binary search in the
//              sorted prefixes; clears the overflow word
//   aggregate  k_gc_bucket_agg: one workgroup per bucket; open-addressing
//              table in LDS (word0, word1, nacc sums, first row), then an
//              ordered emit of the bucket's unique keys into staging arrays
//              at the bucket's own row offset.  <PART = true> reads
//              part_keys[i], part_row[i], part_acc[a][i] in order;
//              <PART = false> reads keys and contributions through perm32.
//   scan       k_gc_bucket_scan: exclusive scan of the per-bucket unique
//              counts; total and overflow word side by side for one read
//   compact    k_gc_bucket_compact (after the host read): staged entries to
//              exact-size outputs, one thread per output entry
//
// Insert protocol, spin-free like k_hash_agg, with a bounded probe count:
// a slot is claimed by a CAS of the row index into its first-row word
// (UNPUB until then).  The winner writes word1 and then, with release
// order, word0 over the bucket's EMPTY value.  Later rows of the key lower
// the first-row word by an atomic min, so at every moment it names a row
// that carries the slot's key.  A thread that meets a claimed slot whose
// words are not yet written therefore neither waits nor probes on blindly:
// it reads the slot's key from that row in global memory.  No thread waits
// on another and a key never owns two slots, so the distinct-key limit is
// exact.  EMPTY needs no reserved key value: every word0 of bucket b
// carries b in its top bits, and EMPTY carries b ^ 1 there.
//
// A workgroup raises the overflow word (ctl[1]) and stages nothing when a
// probe runs past max_probe slots, the bucket has more than max_rows rows
// or more than max_distinct unique keys; the caller then takes the prefix
// path.  Sums are unsigned 64-bit adds and first rows a min, so the result
// does not depend on the order in which rows arrive.

#define PW_GC_BK_THREADS 1024
#define PW_GC_BK_UNPUB 0xFFFFFFFFu
#define PW_GC_BK_LDS_MAX 61440      // dynamic LDS of k_gc_bucket_agg
#define PW_GC_BK_UNROLL 4

// -- the partition: count, scan, scatter --
#define PW_GC_PT_THREADS 1024
#define PW_GC_PT_TILE 8192         // rows per workgroup, count and scatter
#define PW_GC_PT_ROWS (PW_GC_PT_TILE / PW_GC_PT_THREADS)
#define PW_GC_PT_SUB 2048          // rows the staged scatter orders at a time
#define PW_GC_PT_SCAN_RANGES 32    // block ranges of k_gc_part_scan

// bucket id: the top bucket_bits of word0, sign bit flipped (as GcPrefix)
__device__ __forceinline__ uint32_t gc_pt_bucket(unsigned long long w0,
                                                 int drop) {
  return ((uint32_t)(w0 >> 32) ^ 0x80000000u) >> drop;
}

// block_hist rows are padded to 8 entries, so that the scan reads 2 x uint4
static inline uint32_t gc_pt_stride(uint32_t nb) { return nb < 8 ? 8 : nb; }

// blocks per range of k_gc_part_scan
__host__ __device__ static inline uint32_t gc_pt_chunk(uint32_t nblk) {
  return (nblk + PW_GC_PT_SCAN_RANGES - 1) / PW_GC_PT_SCAN_RANGES;
}

__global__ __launch_bounds__(PW_GC_PT_THREADS) void k_gc_part_count(
    const long long* __restrict__ keys, int64_t n, int drop, uint32_t nbp,
    uint32_t* __restrict__ block_hist) {
  __shared__ uint32_t h[256];
  const uint32_t tid = threadIdx.x;
  if (tid < 256) h[tid] = 0;
  __syncthreads();
  const int64_t base = (int64_t)blockIdx.x * PW_GC_PT_TILE + tid;
  unsigned long long w[PW_GC_PT_ROWS];
#pragma unroll
  for (int q = 0; q < PW_GC_PT_ROWS; ++q) {
    const int64_t i = base + (int64_t)q * PW_GC_PT_THREADS;
    w[q] = i < n ? (unsigned long long)keys[2 * (size_t)i] : 0ULL;
  }
#pragma unroll
  for (int q = 0; q < PW_GC_PT_ROWS; ++q) {
    const int64_t i = base + (int64_t)q * PW_GC_PT_THREADS;
    if (i < n) atomicAdd(&h[gc_pt_bucket(w[q], drop)], 1u);
  }
  __syncthreads();
  if (tid < nbp) block_hist[(size_t)blockIdx.x * nbp + tid] = h[tid];
}

// One workgroup.  Thread (tb, tr) owns eight neighbouring buckets and one
// of PW_GC_PT_SCAN_RANGES ranges of blocks and sums its range.  The range
// sums are scanned per bucket and the bucket totals across buckets in LDS.
// Output: bucket_start[0..nb], and range_base[r][b], the first output
// position of range r in bucket b.  block_hist is read once and not
// rewritten (rewriting it with every block's own base made this kernel move
// three times the bytes through one CU: 21 us against 13 us of
// k_gc_part_count at 4M rows); k_gc_part_scatter adds the counts of the at
// most chunk - 1 blocks of its range that come before it.
__global__ __launch_bounds__(PW_GC_PT_THREADS) void k_gc_part_scan(
    const uint32_t* __restrict__ block_hist, uint32_t nblk, uint32_t nb,
    uint32_t nbp, int64_t n, uint32_t* __restrict__ bucket_start,
    uint32_t* __restrict__ range_base, unsigned long long* ctl) {
  __shared__ uint32_t part[PW_GC_PT_SCAN_RANGES][256];
  __shared__ uint32_t sc[256];
  const uint32_t tid = threadIdx.x;
  const uint32_t no = nbp / 8;  // octets of buckets
  const uint32_t tb = tid % no, tr = tid / no;
  const bool active = tr < PW_GC_PT_SCAN_RANGES;
  const uint32_t chunk = gc_pt_chunk(nblk);
  const uint32_t lo = tr * chunk < nblk ? tr * chunk : nblk;
  const uint32_t hi = lo + chunk < nblk ? lo + chunk : nblk;
  const uint4* h4 = (const uint4*)block_hist;
  if (tid == 0) {
    ctl[0] = 0;
    ctl[1] = 0;
  }
  if (active) {
    uint4 s = make_uint4(0, 0, 0, 0), t = make_uint4(0, 0, 0, 0);
#pragma unroll 8
    for (uint32_t blk = lo; blk < hi; ++blk) {
      const uint4 v = h4[((size_t)blk * no + tb) * 2];
      const uint4 w = h4[((size_t)blk * no + tb) * 2 + 1];
      s.x += v.x, s.y += v.y, s.z += v.z, s.w += v.w;
      t.x += w.x, t.y += w.y, t.z += w.z, t.w += w.w;
    }
    uint32_t* p = &part[tr][8 * tb];
    p[0] = s.x, p[1] = s.y, p[2] = s.z, p[3] = s.w;
    p[4] = t.x, p[5] = t.y, p[6] = t.z, p[7] = t.w;
  }
  __syncthreads();
  uint32_t tot = 0;
  if (tid < nbp) {
    for (int r = 0; r < PW_GC_PT_SCAN_RANGES; ++r) {
      const uint32_t v = part[r][tid];
      part[r][tid] = tot;
      tot += v;
    }
  }
  if (tid < 256) sc[tid] = tot;
  __syncthreads();
  for (uint32_t off = 1; off < 256; off <<= 1) {
    const uint32_t v = (tid < 256 && tid >= off) ? sc[tid - off] : 0;
    __syncthreads();
    if (tid < 256) sc[tid] += v;
    __syncthreads();
  }
  if (tid < 256) {
    const uint32_t ex = sc[tid] - tot;
    sc[tid] = ex;  // only this thread reads or writes sc[tid] here
    if (tid < nb) bucket_start[tid] = ex;
  }
  if (tid == 0) bucket_start[nb] = (uint32_t)n;
  __syncthreads();
  for (uint32_t e = tid; e < PW_GC_PT_SCAN_RANGES * nbp; e += PW_GC_PT_THREADS)
    range_base[e] = sc[e % nbp] + part[e / nbp][e % nbp];
}

// STAGED = false: every row goes from registers to the position an LDS
// cursor of its bucket hands out.  STAGED = true: PW_GC_PT_SUB rows at a
// time are first ordered by bucket in LDS, so that a bucket's share of them
// leaves as one contiguous run of 16-B, 8-B and 4-B stores.
template <bool STAGED>
__global__ __launch_bounds__(PW_GC_PT_THREADS) void k_gc_part_scatter(
    const long long* __restrict__ keys, AccPtrs contribs, int nacc, int64_t n,
    int drop, uint32_t nbp, const uint32_t* __restrict__ block_hist,
    const uint32_t* __restrict__ range_base, long long* __restrict__ part_keys,
    uint32_t* __restrict__ part_row, AccPtrsMut part_acc) {
  __shared__ uint32_t cur[256];  // next output position per bucket
  const uint32_t tid = threadIdx.x;
  const ulonglong2* __restrict__ k2 = (const ulonglong2*)keys;
  ulonglong2* __restrict__ o2 = (ulonglong2*)part_keys;
  const long long* __restrict__ c0 = contribs.p[0];
  const int64_t tile = (int64_t)blockIdx.x * PW_GC_PT_TILE;
  if (tid < nbp) {
    // this block's first position: its range's, plus the blocks before it
    const uint32_t chunk = gc_pt_chunk(gridDim.x);
    const uint32_t r = blockIdx.x / chunk;
    uint32_t v = range_base[r * nbp + tid];
    for (uint32_t blk = r * chunk; blk < blockIdx.x; ++blk)
      v += block_hist[(size_t)blk * nbp + tid];
    cur[tid] = v;
  }
  if constexpr (!STAGED) {
    __syncthreads();
    for (int g = 0; g < PW_GC_PT_ROWS; g += 4) {
      ulonglong2 kv[4];
      long long v0[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int64_t i = tile + (int64_t)(g + q) * PW_GC_PT_THREADS + tid;
        if (i < n) {
          kv[q] = k2[i];
          v0[q] = nacc > 0 ? c0[i] : 0;
        }
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int64_t i = tile + (int64_t)(g + q) * PW_GC_PT_THREADS + tid;
        if (i >= n) continue;
        const uint32_t dst = atomicAdd(&cur[gc_pt_bucket(kv[q].x, drop)], 1u);
        o2[dst] = kv[q];
        part_row[dst] = (uint32_t)i;
        if (nacc > 0) part_acc.p[0][dst] = v0[q];
        for (int a = 1; a < nacc; ++a) part_acc.p[a][dst] = contribs.p[a][i];
      }
    }
  } else {
    constexpr int SQ = PW_GC_PT_SUB / PW_GC_PT_THREADS;  // rows per thread
    __shared__ ulonglong2 bufk[PW_GC_PT_SUB];
    __shared__ long long bufa[PW_GC_PT_SUB];
    __shared__ uint32_t bufr[PW_GC_PT_SUB];
    __shared__ uint8_t bkt[PW_GC_PT_SUB];
    __shared__ uint32_t cnt[256], lstart[256], delta[256], wtot[4];
    for (int64_t sbase = tile; sbase < tile + PW_GC_PT_TILE && sbase < n;
         sbase += PW_GC_PT_SUB) {
      const uint32_t m =
          n - sbase < PW_GC_PT_SUB ? (uint32_t)(n - sbase) : PW_GC_PT_SUB;
      if (tid < 256) cnt[tid] = 0;
      __syncthreads();
      ulonglong2 kv[SQ];
      long long v0[SQ];
      uint32_t bk[SQ], lp[SQ];
#pragma unroll
      for (int q = 0; q < SQ; ++q) {
        const uint32_t j = q * PW_GC_PT_THREADS + tid;
        if (j < m) {
          kv[q] = k2[sbase + j];
          v0[q] = nacc > 0 ? c0[sbase + j] : 0;
        }
      }
#pragma unroll
      for (int q = 0; q < SQ; ++q) {
        const uint32_t j = q * PW_GC_PT_THREADS + tid;
        if (j < m) {
          bk[q] = gc_pt_bucket(kv[q].x, drop);
          lp[q] = atomicAdd(&cnt[bk[q]], 1u);  // rank inside the bucket
        }
      }
      __syncthreads();
      // exclusive scan of the 256 counts: four waves, then their totals
      uint32_t c = 0, inc = 0;
      if (tid < 256) {
        c = cnt[tid];
        inc = c;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
          const uint32_t up = __shfl_up(inc, d);
          if ((tid & 63) >= (uint32_t)d) inc += up;
        }
        if ((tid & 63) == 63) wtot[tid >> 6] = inc;
      }
      __syncthreads();
      if (tid < 256) {
        uint32_t off = 0;
        for (uint32_t w = 0; w < (tid >> 6); ++w) off += wtot[w];
        const uint32_t ex = off + inc - c;
        lstart[tid] = ex;
        delta[tid] = cur[tid] - ex;  // output position = delta + LDS position
        cur[tid] += c;
      }
      __syncthreads();
#pragma unroll
      for (int q = 0; q < SQ; ++q) {
        const uint32_t j = q * PW_GC_PT_THREADS + tid;
        if (j < m) {
          lp[q] += lstart[bk[q]];
          bufk[lp[q]] = kv[q];
          bufr[lp[q]] = (uint32_t)(sbase + j);
          bkt[lp[q]] = (uint8_t)bk[q];
          if (nacc > 0) bufa[lp[q]] = v0[q];
        }
      }
      __syncthreads();
#pragma unroll
      for (int q = 0; q < SQ; ++q) {
        const uint32_t j = q * PW_GC_PT_THREADS + tid;
        if (j < m) {
          const uint32_t dst = delta[bkt[j]] + j;
          o2[dst] = bufk[j];
          part_row[dst] = bufr[j];
          if (nacc > 0) part_acc.p[0][dst] = bufa[j];
        }
      }
      for (int a = 1; a < nacc; ++a) {
        __syncthreads();
#pragma unroll
        for (int q = 0; q < SQ; ++q) {
          const uint32_t j = q * PW_GC_PT_THREADS + tid;
          if (j < m) bufa[lp[q]] = contribs.p[a][sbase + j];
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < SQ; ++q) {
          const uint32_t j = q * PW_GC_PT_THREADS + tid;
          if (j < m) part_acc.p[a][delta[bkt[j]] + j] = bufa[j];
        }
      }
    }
  }
}

__global__ void k_gc_bucket_bounds(const uint32_t* __restrict__ prefix_sorted,
                                   int64_t n, uint32_t nb,
                                   uint32_t* bucket_start,
                                   unsigned long long* ctl) {
  uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b == 0) {
    ctl[0] = 0;
    ctl[1] = 0;
  }
  if (b > nb) return;
  int64_t lo = 0, hi = n;  // first position whose prefix is >= b
  while (lo < hi) {
    int64_t mid = (lo + hi) >> 1;
    if (prefix_sorted[mid] < b) lo = mid + 1;
    else hi = mid;
  }
  bucket_start[b] = (uint32_t)lo;
}

__device__ __forceinline__ uint32_t gc_bk_hash(unsigned long long w0,
                                               long long w1, int lg_cap) {
  uint32_t h = (uint32_t)w0 ^ (uint32_t)(w0 >> 29) ^
               ((uint32_t)w1 * 0x9E3779B1u);
  return (h * 0x85EBCA6Bu) >> (32 - lg_cap);
}

// PART = false: perm32 lists the rows of every bucket; keys and contribs are
// the caller's arrays, read through it (NV = 1: the first contribution is
// loaded with the key, the others when the slot is found).
// PART = true: perm32 is part_row, part_keys the partitioned keys, contribs
// the partitioned columns, all read at position i; NV is the number of
// columns held in registers (1 or 8, at least nacc).  keys stays the
// caller's array: slots are claimed with the original row index, and the
// rare read of a claimed slot's key goes there.
template <bool PART, int NV>
__global__ __launch_bounds__(PW_GC_BK_THREADS) void k_gc_bucket_agg(
    const long long* __restrict__ keys, const uint32_t* __restrict__ perm32,
    const long long* __restrict__ part_keys,
    const uint32_t* __restrict__ bucket_start, AccPtrs contribs, int nacc,
    int bucket_bits, uint32_t cap, int lg_cap, uint32_t max_distinct,
    uint32_t max_rows, uint32_t max_probe, long long* st_k0, long long* st_k1,
    uint32_t* st_first, AccPtrsMut st_accs, uint32_t* bucket_uniques,
    unsigned long long* ctl) {
  extern __shared__ unsigned long long gcb_lds[];
  unsigned long long* t0 = gcb_lds;                        // [cap]
  long long* t1 = (long long*)(t0 + cap);                  // [cap]
  unsigned long long* tacc = (unsigned long long*)(t1 + cap);  // [nacc][cap]
  uint32_t* tfirst = (uint32_t*)(tacc + (size_t)nacc * cap);   // [cap]
  uint16_t* list = (uint16_t*)(tfirst + cap);                  // [cap]
  __shared__ uint32_t s_cnt, s_claims, s_ovf;

  const uint32_t b = blockIdx.x;
  const uint32_t tid = threadIdx.x;
  const uint32_t beg = bucket_start[b], end = bucket_start[b + 1];
  const uint32_t rows = end - beg;
  if (rows == 0 || rows > max_rows) {
    if (tid == 0) {
      bucket_uniques[b] = 0;
      if (rows) ctl[1] = 1;
    }
    return;
  }
  const uint32_t mask = cap - 1;
  const unsigned long long empty =
      (unsigned long long)((b ^ 1u) ^ (1u << (bucket_bits - 1)))
      << (64 - bucket_bits);
  for (uint32_t s = tid; s < cap; s += PW_GC_BK_THREADS) {
    t0[s] = empty;
    tfirst[s] = PW_GC_BK_UNPUB;
    for (int a = 0; a < nacc; ++a) tacc[(size_t)a * cap + s] = 0;
  }
  if (tid == 0) s_cnt = 0, s_claims = 0, s_ovf = 0;
  __syncthreads();

  const long long* c0 = contribs.p[0];
  for (int64_t base = (int64_t)beg + tid; base < (int64_t)end;
       base += (int64_t)PW_GC_BK_UNROLL * PW_GC_BK_THREADS) {
    uint32_t row[PW_GC_BK_UNROLL];
    unsigned long long k0[PW_GC_BK_UNROLL];
    long long k1[PW_GC_BK_UNROLL];
    unsigned long long v[PW_GC_BK_UNROLL][NV];
#pragma unroll
    for (int q = 0; q < PW_GC_BK_UNROLL; ++q) {
      int64_t i = base + (int64_t)q * PW_GC_BK_THREADS;
      row[q] = i < (int64_t)end ? perm32[i] : PW_GC_BK_UNPUB;
    }
#pragma unroll
    for (int q = 0; q < PW_GC_BK_UNROLL; ++q) {
      if (row[q] == PW_GC_BK_UNPUB) continue;
      if constexpr (PART) {
        const int64_t i = base + (int64_t)q * PW_GC_BK_THREADS;
        const ulonglong2 kv = ((const ulonglong2*)part_keys)[i];
        k0[q] = kv.x;
        k1[q] = (long long)kv.y;
#pragma unroll
        for (int a = 0; a < NV; ++a)
          v[q][a] = a < nacc ? (unsigned long long)contribs.p[a][i] : 0ULL;
      } else {
        k0[q] = (unsigned long long)keys[2 * (size_t)row[q]];
        k1[q] = keys[2 * (size_t)row[q] + 1];
        v[q][0] = nacc > 0 ? (unsigned long long)c0[row[q]] : 0ULL;
      }
    }
#pragma unroll
    for (int q = 0; q < PW_GC_BK_UNROLL; ++q) {
      if (row[q] == PW_GC_BK_UNPUB) continue;
      // once the bucket has overflowed the rest of its rows is not needed
      if (__hip_atomic_load(&s_ovf, __ATOMIC_RELAXED,
                            __HIP_MEMORY_SCOPE_WORKGROUP))
        break;
      const unsigned long long key0 = k0[q];
      const long long key1 = k1[q];
      uint32_t slot = gc_bk_hash(key0, key1, lg_cap);
      bool done = false;
      for (uint32_t tries = 0; tries < max_probe; ++tries) {
        bool match;
        const unsigned long long cur = __hip_atomic_load(
            &t0[slot], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (cur != empty) {
          match = cur == key0 && t1[slot] == key1;
          if (match) atomicMin(&tfirst[slot], row[q]);
        } else {
          const uint32_t f = atomicCAS(&tfirst[slot], PW_GC_BK_UNPUB, row[q]);
          match = f == PW_GC_BK_UNPUB;
          if (match) {
            // claimed: word1, then word0 with release order
            if (atomicAdd(&s_claims, 1u) >= max_distinct) s_ovf = 1;
            t1[slot] = key1;
            __hip_atomic_store(&t0[slot], key0, __ATOMIC_RELEASE,
                               __HIP_MEMORY_SCOPE_WORKGROUP);
          } else {
            // claimed, words not written yet: row f carries the slot's key
            match = (unsigned long long)keys[2 * (size_t)f] == key0 &&
                    keys[2 * (size_t)f + 1] == key1;
            if (match) atomicMin(&tfirst[slot], row[q]);
          }
        }
        if (match) {
          if (nacc > 0) atomicAdd(&tacc[slot], v[q][0]);
          if constexpr (PART) {
#pragma unroll
            for (int a = 1; a < NV; ++a)
              if (a < nacc) atomicAdd(&tacc[(size_t)a * cap + slot], v[q][a]);
          } else {
            for (int a = 1; a < nacc; ++a)
              atomicAdd(&tacc[(size_t)a * cap + slot],
                        (unsigned long long)contribs.p[a][row[q]]);
          }
          done = true;
          break;
        }
        slot = (slot + 1) & mask;
      }
      if (!done) s_ovf = 1;
    }
  }
  __syncthreads();

  // occupied slots, in any order
  for (uint32_t s = tid; s < cap; s += PW_GC_BK_THREADS)
    if (tfirst[s] != PW_GC_BK_UNPUB) list[atomicAdd(&s_cnt, 1u)] = (uint16_t)s;
  __syncthreads();
  const uint32_t cnt = s_cnt;  // the bucket's distinct keys
  if (s_ovf || cnt > max_distinct) {
    if (tid == 0) {
      bucket_uniques[b] = 0;
      ctl[1] = 1;
    }
    return;
  }

  // rank sort by (word0, word1), signed; cnt <= rows, so beg + rank stays
  // inside the bucket's own rows of the staging arrays
  for (uint32_t t = tid; t < cnt; t += PW_GC_BK_THREADS) {
    const uint32_t sl = list[t];
    const long long a0 = (long long)t0[sl], a1 = t1[sl];
    uint32_t rank = 0;
    for (uint32_t u = 0; u < cnt; ++u) {
      const uint32_t su = list[u];
      const long long b0 = (long long)t0[su];
      rank += (b0 < a0 || (b0 == a0 && t1[su] < a1)) ? 1u : 0u;
    }
    const size_t o = (size_t)beg + rank;
    st_k0[o] = a0;
    st_k1[o] = a1;
    st_first[o] = tfirst[sl];
    for (int a = 0; a < nacc; ++a)
      st_accs.p[a][o] = (long long)tacc[(size_t)a * cap + sl];
  }
  if (tid == 0) bucket_uniques[b] = cnt;
}

// one block: base[0..nb] = exclusive scan of uniq[0..nb), ctl[0] = total
__global__ void k_gc_bucket_scan(const uint32_t* __restrict__ uniq,
                                 uint32_t nb, long long* base,
                                 unsigned long long* ctl) {
  __shared__ long long part[PW_BLOCK];
  const uint32_t tid = threadIdx.x;
  const uint32_t chunk = (nb + PW_BLOCK - 1) / PW_BLOCK;
  const uint32_t lo = tid * chunk < nb ? tid * chunk : nb;
  const uint32_t hi = lo + chunk < nb ? lo + chunk : nb;
  long long sum = 0;
  for (uint32_t i = lo; i < hi; ++i) sum += uniq[i];
  part[tid] = sum;
  __syncthreads();
  for (uint32_t off = 1; off < PW_BLOCK; off <<= 1) {
    long long v = tid >= off ? part[tid - off] : 0;
    __syncthreads();
    part[tid] += v;
    __syncthreads();
  }
  long long run = part[tid] - sum;  // exclusive
  for (uint32_t i = lo; i < hi; ++i) {
    base[i] = run;
    run += uniq[i];
  }
  if (tid == PW_BLOCK - 1) {
    base[nb] = part[tid];
    ctl[0] = (unsigned long long)part[tid];
  }
}

__global__ void k_gc_bucket_compact(const long long* __restrict__ base,
                                    const uint32_t* __restrict__ bucket_start,
                                    uint32_t nb, int64_t total,
                                    const long long* __restrict__ st_k0,
                                    const long long* __restrict__ st_k1,
                                    const uint32_t* __restrict__ st_first,
                                    AccPtrs st_accs, int nacc,
                                    long long* out_k0, long long* out_k1,
                                    long long* out_first,
                                    AccPtrsMut out_accs) {
  int64_t o = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (o >= total) return;
  uint32_t lo = 0, hi = nb - 1;  // last bucket whose base is <= o
  while (lo < hi) {
    uint32_t mid = (lo + hi + 1) >> 1;
    if (base[mid] <= o) lo = mid;
    else hi = mid - 1;
  }
  size_t src = (size_t)bucket_start[lo] + (size_t)(o - base[lo]);
  out_k0[o] = st_k0[src];
  out_k1[o] = st_k1[src];
  out_first[o] = (long long)st_first[src];
  for (int a = 0; a < nacc; ++a) out_accs.p[a][o] = st_accs.p[a][src];
}

// LDS bytes k_gc_bucket_agg needs per table entry
static inline size_t gc_bk_entry_bytes(int nacc) {
  return 8 + 8 + 8 * (size_t)nacc + 4 + 2;
}

// largest power-of-two table capacity that fits the kernel's LDS (0 if none)
extern "C" int64_t pw_gc_bucket_max_capacity(int nacc) {
  if (nacc < 0 || nacc > 8) return 0;
  int64_t cap = 1;
  while ((size_t)(2 * cap) * gc_bk_entry_bytes(nacc) <= PW_GC_BK_LDS_MAX)
    cap *= 2;
  return cap;
}

// partition + bounds + aggregate + scan on the caller's stream.  keys: (n,2)
// int64 rows 16 B apart.  prefix_scratch, perm32, st_first: n uint32;
// st_k0, st_k1, st_accs[a]: n int64; bucket_start: nb+1 uint32;
// bucket_uniques: nb uint32; base: nb+1 int64; ctl: 2 uint64 (total unique
// keys, overflow word), nb = 2^bucket_bits.
extern "C" int pw_gc_bucket_agg(const void* keys, int64_t n, void* temp,
                                int64_t temp_bytes, void* prefix_scratch,
                                void* perm32, int bucket_bits,
                                int64_t table_capacity, int64_t max_distinct,
                                int64_t max_bucket_rows, int64_t max_probe,
                                const void** contrib_ptrs, int nacc,
                                void* bucket_start, void* bucket_uniques,
                                void* base, void* st_k0, void* st_k1,
                                void* st_first, void** st_acc_ptrs, void* ctl,
                                void* stream) {
  if (n < 2 || n >= ((int64_t)1 << 32) - 1) return 1;
  if (bucket_bits < 1 || bucket_bits > 16) return 1;
  if (nacc < 0 || nacc > 8) return 1;
  if (table_capacity < 2 || table_capacity > 32768 ||
      (table_capacity & (table_capacity - 1)))
    return 1;
  size_t lds = (size_t)table_capacity * gc_bk_entry_bytes(nacc);
  if (lds > PW_GC_BK_LDS_MAX) return 1;
  if (max_distinct < 1 || max_distinct > table_capacity) return 1;
  if (max_bucket_rows < 1 || max_probe < 1) return 1;
  if (max_bucket_rows > 0xFFFFFFFFLL) max_bucket_rows = 0xFFFFFFFFLL;
  if (max_probe > table_capacity) max_probe = table_capacity;
  int lg_cap = 0;
  while (((int64_t)1 << lg_cap) < table_capacity) ++lg_cap;
  hipStream_t s = (hipStream_t)stream;
  size_t tb = (size_t)temp_bytes;
  hipError_t e = gc_sort_prefix(temp, tb, (const long long*)keys,
                                (uint32_t*)prefix_scratch, (uint32_t*)perm32,
                                n, bucket_bits, s);
  if (e != hipSuccess) return (int)e;
  AccPtrs cp;
  AccPtrsMut sp;
  for (int a = 0; a < 8; ++a) {
    cp.p[a] = a < nacc ? (const long long*)contrib_ptrs[a] : nullptr;
    sp.p[a] = a < nacc ? (long long*)st_acc_ptrs[a] : nullptr;
  }
  uint32_t nb = 1u << bucket_bits;
  hipLaunchKernelGGL(k_gc_bucket_bounds,
                     dim3((nb + 1 + PW_BLOCK - 1) / PW_BLOCK), dim3(PW_BLOCK),
                     0, s, (const uint32_t*)prefix_scratch, n, nb,
                     (uint32_t*)bucket_start, (unsigned long long*)ctl);
  hipLaunchKernelGGL((k_gc_bucket_agg<false, 1>), dim3(nb),
                     dim3(PW_GC_BK_THREADS), lds, s, (const long long*)keys,
                     (const uint32_t*)perm32, (const long long*)nullptr,
                     (const uint32_t*)bucket_start, cp, nacc, bucket_bits,
                     (uint32_t)table_capacity, lg_cap, (uint32_t)max_distinct,
                     (uint32_t)max_bucket_rows, (uint32_t)max_probe,
                     (long long*)st_k0, (long long*)st_k1, (uint32_t*)st_first,
                     sp, (uint32_t*)bucket_uniques, (unsigned long long*)ctl);
  hipLaunchKernelGGL(k_gc_bucket_scan, dim3(1), dim3(PW_BLOCK), 0, s,
                     (const uint32_t*)bucket_uniques, nb, (long long*)base,
                     (unsigned long long*)ctl);
  return (int)hipGetLastError();
}

// rows per workgroup of the partition kernels
extern "C" int64_t pw_gc_part_tile() { return PW_GC_PT_TILE; }

// uint32 entries of block_hist, with the scan's range_base behind it, for n
// rows (0: not a partition case)
extern "C" int64_t pw_gc_part_hist_entries(int64_t n, int bucket_bits) {
  if (n < 2 || n >= ((int64_t)1 << 32) - 1) return 0;
  if (bucket_bits < 1 || bucket_bits > 8) return 0;
  int64_t nblk = (n + PW_GC_PT_TILE - 1) / PW_GC_PT_TILE;
  return (nblk + PW_GC_PT_SCAN_RANGES) *
         (int64_t)gc_pt_stride(1u << bucket_bits);
}

// count + scan + scatter on stream s; arguments checked by the callers
static void gc_partition_launch(const long long* keys, int64_t n,
                                int bucket_bits, const AccPtrs& cp, int nacc,
                                uint32_t* block_hist, long long* part_keys,
                                uint32_t* part_row, const AccPtrsMut& pp,
                                uint32_t* bucket_start,
                                unsigned long long* ctl, int direct,
                                hipStream_t s) {
  const uint32_t nb = 1u << bucket_bits, nbp = gc_pt_stride(nb);
  const uint32_t nblk = (uint32_t)((n + PW_GC_PT_TILE - 1) / PW_GC_PT_TILE);
  const int drop = 32 - bucket_bits;
  uint32_t* range_base = block_hist + (size_t)nblk * nbp;
  hipLaunchKernelGGL(k_gc_part_count, dim3(nblk), dim3(PW_GC_PT_THREADS), 0, s,
                     keys, n, drop, nbp, block_hist);
  hipLaunchKernelGGL(k_gc_part_scan, dim3(1), dim3(PW_GC_PT_THREADS), 0, s,
                     (const uint32_t*)block_hist, nblk, nb, nbp, n,
                     bucket_start, range_base, ctl);
  if (direct)
    hipLaunchKernelGGL(k_gc_part_scatter<false>, dim3(nblk),
                       dim3(PW_GC_PT_THREADS), 0, s, keys, cp, nacc, n, drop,
                       nbp, (const uint32_t*)block_hist,
                       (const uint32_t*)range_base, part_keys, part_row, pp);
  else
    hipLaunchKernelGGL(k_gc_part_scatter<true>, dim3(nblk),
                       dim3(PW_GC_PT_THREADS), 0, s, keys, cp, nacc, n, drop,
                       nbp, (const uint32_t*)block_hist,
                       (const uint32_t*)range_base, part_keys, part_row, pp);
}

static bool gc_partition_args_ok(const void* keys, int64_t n, int bucket_bits,
                                 int nacc, const void* block_hist,
                                 const void* part_keys) {
  if (n < 2 || n >= ((int64_t)1 << 32) - 1) return false;
  if (bucket_bits < 1 || bucket_bits > 8) return false;
  if (nacc < 0 || nacc > 8) return false;
  // 128-bit loads and stores
  return ((uintptr_t)keys | (uintptr_t)block_hist | (uintptr_t)part_keys) % 16 == 0;
}

// The partition alone (tests).  keys: (n,2) int64, 16-B aligned; block_hist:
// pw_gc_part_hist_entries uint32, 16-B aligned; part_keys: (n,2) int64;
// part_row: n uint32; part_acc[a]: n int64; bucket_start: nb+1 uint32; ctl:
// 2 uint64, cleared.  direct != 0 scatters from registers (A/B runs).
extern "C" int pw_gc_partition(const void* keys, int64_t n, int bucket_bits,
                               const void** contrib_ptrs, int nacc,
                               void* block_hist, void* part_keys,
                               void* part_row, void** part_acc_ptrs,
                               void* bucket_start, void* ctl, int direct,
                               void* stream) {
  if (!gc_partition_args_ok(keys, n, bucket_bits, nacc, block_hist, part_keys))
    return 1;
  AccPtrs cp;
  AccPtrsMut pp;
  for (int a = 0; a < 8; ++a) {
    cp.p[a] = a < nacc ? (const long long*)contrib_ptrs[a] : nullptr;
    pp.p[a] = a < nacc ? (long long*)part_acc_ptrs[a] : nullptr;
  }
  gc_partition_launch((const long long*)keys, n, bucket_bits, cp, nacc,
                      (uint32_t*)block_hist, (long long*)part_keys,
                      (uint32_t*)part_row, pp, (uint32_t*)bucket_start,
                      (unsigned long long*)ctl, direct, (hipStream_t)stream);
  return (int)hipGetLastError();
}

// pw_gc_bucket_agg on the partition layout (bucket_bits <= 8): partition +
// aggregate + scan on the caller's stream; no temp, prefix scratch or
// perm32.  Partition arguments as pw_gc_partition, the others as
// pw_gc_bucket_agg; pw_gc_bucket_compact follows the same host read.
extern "C" int pw_gc_bucket_part_agg(
    const void* keys, int64_t n, int bucket_bits, int64_t table_capacity,
    int64_t max_distinct, int64_t max_bucket_rows, int64_t max_probe,
    const void** contrib_ptrs, int nacc, void* block_hist, void* part_keys,
    void* part_row, void** part_acc_ptrs, void* bucket_start,
    void* bucket_uniques, void* base, void* st_k0, void* st_k1, void* st_first,
    void** st_acc_ptrs, void* ctl, int direct, void* stream) {
  if (!gc_partition_args_ok(keys, n, bucket_bits, nacc, block_hist, part_keys))
    return 1;
  if (table_capacity < 2 || table_capacity > 32768 ||
      (table_capacity & (table_capacity - 1)))
    return 1;
  size_t lds = (size_t)table_capacity * gc_bk_entry_bytes(nacc);
  if (lds > PW_GC_BK_LDS_MAX) return 1;
  if (max_distinct < 1 || max_distinct > table_capacity) return 1;
  if (max_bucket_rows < 1 || max_probe < 1) return 1;
  if (max_bucket_rows > 0xFFFFFFFFLL) max_bucket_rows = 0xFFFFFFFFLL;
  if (max_probe > table_capacity) max_probe = table_capacity;
  int lg_cap = 0;
  while (((int64_t)1 << lg_cap) < table_capacity) ++lg_cap;
  hipStream_t s = (hipStream_t)stream;
  AccPtrs cp, pc;
  AccPtrsMut pp, sp;
  for (int a = 0; a < 8; ++a) {
    cp.p[a] = a < nacc ? (const long long*)contrib_ptrs[a] : nullptr;
    pp.p[a] = a < nacc ? (long long*)part_acc_ptrs[a] : nullptr;
    pc.p[a] = pp.p[a];
    sp.p[a] = a < nacc ? (long long*)st_acc_ptrs[a] : nullptr;
  }
  gc_partition_launch((const long long*)keys, n, bucket_bits, cp, nacc,
                      (uint32_t*)block_hist, (long long*)part_keys,
                      (uint32_t*)part_row, pp, (uint32_t*)bucket_start,
                      (unsigned long long*)ctl, direct, s);
  const uint32_t nb = 1u << bucket_bits;
  auto agg = nacc <= 1 ? k_gc_bucket_agg<true, 1> : k_gc_bucket_agg<true, 8>;
  hipLaunchKernelGGL(agg, dim3(nb), dim3(PW_GC_BK_THREADS), lds, s,
                     (const long long*)keys, (const uint32_t*)part_row,
                     (const long long*)part_keys,
                     (const uint32_t*)bucket_start, pc, nacc, bucket_bits,
                     (uint32_t)table_capacity, lg_cap, (uint32_t)max_distinct,
                     (uint32_t)max_bucket_rows, (uint32_t)max_probe,
                     (long long*)st_k0, (long long*)st_k1, (uint32_t*)st_first,
                     sp, (uint32_t*)bucket_uniques, (unsigned long long*)ctl);
  hipLaunchKernelGGL(k_gc_bucket_scan, dim3(1), dim3(PW_BLOCK), 0, s,
                     (const uint32_t*)bucket_uniques, nb, (long long*)base,
                     (unsigned long long*)ctl);
  return (int)hipGetLastError();
}

extern "C" int pw_gc_bucket_compact(const void* base, const void* bucket_start,
                                    int bucket_bits, int64_t total,
                                    const void* st_k0, const void* st_k1,
                                    const void* st_first,
                                    const void** st_acc_ptrs, int nacc,
                                    void* out_k0, void* out_k1,
                                    void* out_first, void** out_acc_ptrs,
                                    void* stream) {
  if (bucket_bits < 1 || bucket_bits > 16 || nacc < 0 || nacc > 8) return 1;
  if (total < 1) return 0;
  AccPtrs sp;
  AccPtrsMut op;
  for (int a = 0; a < 8; ++a) {
    sp.p[a] = a < nacc ? (const long long*)st_acc_ptrs[a] : nullptr;
    op.p[a] = a < nacc ? (long long*)out_acc_ptrs[a] : nullptr;
  }
  int64_t nblocks = (total + PW_BLOCK - 1) / PW_BLOCK;
  hipLaunchKernelGGL(k_gc_bucket_compact, dim3((uint32_t)nblocks),
                     dim3(PW_BLOCK), 0, (hipStream_t)stream,
                     (const long long*)base, (const uint32_t*)bucket_start,
                     1u << bucket_bits, total, (const long long*)st_k0,
                     (const long long*)st_k1, (const uint32_t*)st_first, sp,
                     nacc, (long long*)out_k0, (long long*)out_k1,
                     (long long*)out_first, op);
  return (int)hipGetLastError();
}

template <bool POS>
static int gc_emit_launch(const void* k0_sorted, const void* k1_sorted,
                          const void* perm32, const void** contrib_ptrs,
                          int nacc, int64_t n, const void* block_csum,
                          void* out_k0, void* out_k1, void* out_first,
                          void** out_acc_ptrs, void* out_pos, void* stream) {
  if (nacc < 0 || nacc > 8 || n < 1) return 1;
  AccPtrs cp;
  AccPtrsMut op;
  for (int a = 0; a < nacc; ++a) {
    cp.p[a] = (const long long*)contrib_ptrs[a];
    op.p[a] = (long long*)out_acc_ptrs[a];
  }
  hipStream_t s = (hipStream_t)stream;
  int64_t nblocks = (n + PW_BLOCK - 1) / PW_BLOCK;
  hipLaunchKernelGGL(k_gc_emit<POS>, dim3((uint32_t)nblocks), dim3(PW_BLOCK),
                     0, s, (const long long*)k0_sorted,
                     (const long long*)k1_sorted, (const uint32_t*)perm32, cp,
                     nacc, n, (const long long*)block_csum,
                     (long long*)out_k0, (long long*)out_k1,
                     (long long*)out_first, op, (long long*)out_pos);
  return (int)hipGetLastError();
}

extern "C" int pw_gc_emit(const void* k0_sorted, const void* k1_sorted,
                          const void* perm32, const void** contrib_ptrs,
                          int nacc, int64_t n, const void* block_csum,
                          void* out_k0, void* out_k1, void* out_first,
                          void** out_acc_ptrs, void* stream) {
  return gc_emit_launch<false>(k0_sorted, k1_sorted, perm32, contrib_ptrs,
                               nacc, n, block_csum, out_k0, out_k1, out_first,
                               out_acc_ptrs, nullptr, stream);
}

// pw_gc_emit that also writes seg_pos (nseg + 1 int64): every segment's
// start position in sorted order, then n (the mixed combiner's input to
// pw_seg_sum_f64)
extern "C" int pw_gc_emit_pos(const void* k0_sorted, const void* k1_sorted,
                              const void* perm32, const void** contrib_ptrs,
                              int nacc, int64_t n, const void* block_csum,
                              void* out_k0, void* out_k1, void* out_first,
                              void** out_acc_ptrs, void* seg_pos,
                              void* stream) {
  if (seg_pos == nullptr) return 1;
  return gc_emit_launch<true>(k0_sorted, k1_sorted, perm32, contrib_ptrs,
                              nacc, n, block_csum, out_k0, out_k1, out_first,
                              out_acc_ptrs, seg_pos, stream);
}

// -------------------------------------------------- output consolidation --
// consolidate_batch on the device, start to finish: rows of (key128,
// columns..., diff) -> the rows that survive, with their summed diffs.
//
//   ident    k_row_ident: the 128-bit row identity (c0, c1) of every row,
//            interleaved, in one pass (contract below)
//   group    pw_gc_prefix_sort_count on the identities: prefix sort, gather,
//            mark, repair, segment count (group combine, prefix sort, above)
//   scan     k_cr_scan: inclusive scan of the block counts, in one block
//   emit     k_cr_emit: k_gc_emit for one sum, without the key outputs
//   nonzero  k_cr_nz<false>, k_cr_scan, k_cr_nz<true>: count, scan and
//            compact the identities whose diffs do not sum to zero
//
// Every buffer is sized by n, so nothing on this path waits for a count:
// the caller reads ctl once at the end and narrows rows / wsum to ctl[2].
//
// Ordering contract: rows[j] is the smallest input row of the j-th
// surviving identity and wsum[j] its summed diff; identities ascend in
// signed lexicographic (c0, c1) order, the order that a stable sort of c0
// with word1 ties repaired gives.  Rows are grouped by (c0, c1) itself, not
// by comparing (key, value hash) among neighbours: two different rows fall
// together only where two 128-bit hashes collide, and the engine takes
// 128-bit hashes for identities everywhere (the value hash is one).
//
// ctl (4 x uint64): [0] overflow of the prefix repair (the caller then
// groups the identities with the 64-bit sort), [1] prefix runs listed,
// [2] surviving identities, [3] identities.

#define PW_RI_INT64_TAGGED 0
#define PW_RI_POOL_CODE 1
#define PW_RI_POINTER 2
#define PW_RI_PRECOMPUTED 3
#define PW_RI_MAX_COLS 10

// One column of a row.  By kind:
//   INT64_TAGGED  a = int64 payload, b = bool validity mask or null, x = tag
//   POOL_CODE     a = int64 codes, b / c = the pool's lo / hi hash tables
//   POINTER       a = (n,2) int64 pairs, x = the pointer tag
//   PRECOMPUTED   a / b = the column's own lo / hi value hashes
struct RiCol {
  const void* a;
  const void* b;
  const void* c;
  uint64_t x;
  int kind;
};

struct RiCols {
  RiCol c[PW_RI_MAX_COLS];
};

// Hash contract.  Per column the value hash (lo, hi) is
//   INT64_TAGGED  hash128([tag, payload]) as k_value_hash; the None hash
//                 where the mask is false
//   POOL_CODE     (pool_lo[code], pool_hi[code]); the None hash for code < 0,
//                 as k_pool_hash
//   POINTER       hash128([tag, lo, hi])
//   PRECOMPUTED   as given
// then v = hash128([lo_0, hi_0, lo_1, hi_1, ...]) in column order, (0, 0)
// without columns, and (c0, c1) = hash128([k0, k1, v0, v1]), written to
// ckeys[2i], ckeys[2i + 1].  hash128 is (xxh64 seed LO, xxh64 seed HI) over
// the words, as k_hash128_words: the result is bit-identical to the value
// hashes, combine_value_hashes and hash128_words run one after the other.
// Also clears sums[i], the accumulator k_cr_emit adds into.
template <int NC>
__global__ void k_row_ident(const uint64_t* __restrict__ keys, RiCols cols,
                            uint64_t none_lo, uint64_t none_hi, int64_t n,
                            uint64_t* __restrict__ ckeys,
                            long long* __restrict__ sums) {
  // one row per thread, no grid-stride loop: a loop makes the compiler
  // keep all ten descriptors in scalar registers at once
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) {
    uint64_t c[4];
    c[0] = keys[2 * i];
    c[1] = keys[2 * i + 1];
    c[2] = 0;
    c[3] = 0;
    if (NC > 0) {
      uint64_t w[NC > 0 ? 2 * NC : 2];
#pragma unroll
      for (int j = 0; j < NC; ++j) {
        const RiCol& d = cols.c[j];
        uint64_t lo, hi;
        if (d.kind == PW_RI_INT64_TAGGED) {
          uint64_t t[2] = {d.x, ((const uint64_t*)d.a)[i]};
          lo = pw_xxh64_words<2>(t, PW_SEED_LO);
          hi = pw_xxh64_words<2>(t, PW_SEED_HI);
          if (d.b != nullptr && !((const uint8_t*)d.b)[i]) {
            lo = none_lo;
            hi = none_hi;
          }
        } else if (d.kind == PW_RI_POOL_CODE) {
          int64_t code = ((const int64_t*)d.a)[i];
          lo = none_lo;
          hi = none_hi;
          if (code >= 0) {
            lo = ((const uint64_t*)d.b)[code];
            hi = ((const uint64_t*)d.c)[code];
          }
        } else if (d.kind == PW_RI_POINTER) {
          uint64_t t[3] = {d.x, ((const uint64_t*)d.a)[2 * i],
                           ((const uint64_t*)d.a)[2 * i + 1]};
          lo = pw_xxh64_words<3>(t, PW_SEED_LO);
          hi = pw_xxh64_words<3>(t, PW_SEED_HI);
        } else {
          lo = ((const uint64_t*)d.a)[i];
          hi = ((const uint64_t*)d.b)[i];
        }
        w[2 * j] = lo;
        w[2 * j + 1] = hi;
      }
      c[2] = pw_xxh64_words<(NC > 0 ? 2 * NC : 2)>(w, PW_SEED_LO);
      c[3] = pw_xxh64_words<(NC > 0 ? 2 * NC : 2)>(w, PW_SEED_HI);
    }
    ckeys[2 * i] = pw_xxh64_words<4>(c, PW_SEED_LO);
    ckeys[2 * i + 1] = pw_xxh64_words<4>(c, PW_SEED_HI);
    if (sums != nullptr) sums[i] = 0;
  }
}

static int ri_fill(RiCols& cols, const int* kinds, const void** a,
                   const void** b, const void** c, const uint64_t* x,
                   int ncols) {
  if (ncols < 0 || ncols > PW_RI_MAX_COLS) return 1;
  for (int j = 0; j < PW_RI_MAX_COLS; ++j) {
    RiCol& d = cols.c[j];
    d.a = d.b = d.c = nullptr;
    d.x = 0;
    d.kind = PW_RI_PRECOMPUTED;
    if (j >= ncols) continue;
    if (kinds[j] < PW_RI_INT64_TAGGED || kinds[j] > PW_RI_PRECOMPUTED)
      return 1;
    d.kind = kinds[j];
    d.a = a[j];
    d.b = b[j];
    d.c = c[j];
    d.x = x[j];
    if (d.a == nullptr) return 1;
    if (d.kind == PW_RI_PRECOMPUTED && d.b == nullptr) return 1;
    if (d.kind == PW_RI_POOL_CODE && (d.b == nullptr || d.c == nullptr))
      return 1;
  }
  return 0;
}

static int ri_launch(const void* keys, const RiCols& cols, int ncols,
                     uint64_t none_lo, uint64_t none_hi, int64_t n,
                     void* ckeys, void* sums, hipStream_t s) {
  dim3 grid((uint32_t)((n + PW_BLOCK - 1) / PW_BLOCK)), block(PW_BLOCK);
#define CASE(NC)                                                          \
  case NC:                                                                \
    hipLaunchKernelGGL((k_row_ident<NC>), grid, block, 0, s,              \
                       (const uint64_t*)keys, cols, none_lo, none_hi, n,  \
                       (uint64_t*)ckeys, (long long*)sums);               \
    break;
  switch (ncols) {
    CASE(0) CASE(1) CASE(2) CASE(3) CASE(4) CASE(5) CASE(6) CASE(7)
    CASE(8) CASE(9) CASE(10)
    default:
      return 1;
  }
#undef CASE
  return (int)hipGetLastError();
}

// keys: (n,2) int64 rows 16 B apart; ckeys: (n,2) int64 out.  kinds, a, b,
// c, x: ncols entries each (see RiCol).
extern "C" int pw_row_ident(const void* keys, int64_t n, const int* kinds,
                            const void** a, const void** b, const void** c,
                            const uint64_t* x, int ncols, uint64_t none_lo,
                            uint64_t none_hi, void* ckeys, void* stream) {
  if (n < 1 || n >= ((int64_t)1 << 32)) return 1;
  RiCols cols;
  if (ri_fill(cols, kinds, a, b, c, x, ncols)) return 1;
  return ri_launch(keys, cols, ncols, none_lo, none_hi, n, ckeys, nullptr,
                   (hipStream_t)stream);
}

// Inclusive scan of m int32 counts into int64, one block; the total also
// goes to *total.
#define PW_CR_SCAN_THREADS 1024

__global__ __launch_bounds__(PW_CR_SCAN_THREADS) void k_cr_scan(
    const int* __restrict__ counts, int64_t m, long long* __restrict__ csum,
    unsigned long long* total) {
  __shared__ long long wave_tot[PW_CR_SCAN_THREADS / 64];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  long long carry = 0;
  for (int64_t t0 = 0; t0 < m; t0 += PW_CR_SCAN_THREADS) {
    int64_t i = t0 + tid;
    long long x = (i < m) ? (long long)counts[i] : 0;
    for (int dlt = 1; dlt < 64; dlt <<= 1) {
      long long y = __shfl_up(x, dlt, 64);
      if (lane >= dlt) x += y;
    }
    if (lane == 63) wave_tot[wave] = x;
    __syncthreads();
    long long before = 0, all = 0;
    for (int wv = 0; wv < PW_CR_SCAN_THREADS / 64; ++wv) {
      long long wt = wave_tot[wv];
      if (wv < wave) before += wt;
      all += wt;
    }
    if (i < m) csum[i] = carry + before + x;
    carry += all;
    __syncthreads();
  }
  if (tid == 0) *total = (unsigned long long)carry;
}

// k_gc_emit for one sum and without the key outputs: the first (smallest)
// input row of every (k0, k1) segment and the sum of contrib over its rows,
// added into out_sum (cleared by k_row_ident).  block_csum: inclusive.
__global__ void k_cr_emit(const long long* __restrict__ k0,
                          const long long* __restrict__ k1,
                          const uint32_t* __restrict__ perm32,
                          const long long* __restrict__ contrib, int64_t n,
                          const long long* __restrict__ block_csum,
                          long long* out_first, long long* out_sum) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int lane = threadIdx.x & 63;
  int flag = 0;
  uint32_t row = 0;
  if (i < n) {
    row = perm32[i];
    flag = (i == 0) || k0[i] != k0[i - 1] || k1[i] != k1[i - 1];
  }
  uint64_t ball = __ballot(flag);
  int wave = threadIdx.x >> 6;
  __shared__ int wave_tot[PW_BLOCK / 64];
  if (lane == 0) wave_tot[wave] = __popcll(ball);
  __syncthreads();
  int wave_base = 0;
  for (int j = 0; j < wave; ++j) wave_base += wave_tot[j];
  uint64_t below = ball & ((lane == 0) ? 0ULL : ((1ULL << lane) - 1));
  int local_excl = wave_base + __popcll(below);
  long long base = blockIdx.x ? block_csum[blockIdx.x - 1] : 0;
  long long sid = base + local_excl + flag - 1;
  if (i < n && flag) out_first[sid] = (long long)row;
  // padding lanes carry the sentinel -1, as in k_gc_emit
  long long s = (i < n) ? sid : -1;
  long long nxt = __shfl_down(s, 1, 64);
  bool tail = (lane == 63) || (nxt != s);
  long long v = (i < n) ? contrib[row] : 0;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    long long vv = __shfl_up(v, off, 64);
    long long ss = __shfl_up(s, off, 64);
    if (lane >= off && ss == s) v += vv;
  }
  if (s >= 0 && tail)
    atomicAdd((unsigned long long*)&out_sum[s], (unsigned long long)v);
}

// Identities with a nonzero sum.  WRITE false: their number per block.
// WRITE true: their first rows and sums, compacted in order, and with
// out_keys given the (n,2) keys of those rows; block_csum is the inclusive
// scan of the counts.  *nseg_p: the number of identities.
template <bool WRITE>
__global__ void k_cr_nz(const long long* __restrict__ first,
                        const long long* __restrict__ sums, int64_t n,
                        const unsigned long long* __restrict__ nseg_p,
                        int* block_counts,
                        const long long* __restrict__ block_csum,
                        long long* __restrict__ out_rows,
                        long long* __restrict__ out_w,
                        const long long* __restrict__ keys,
                        long long* __restrict__ out_keys) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t nseg = (int64_t)*nseg_p;
  if (nseg > n) nseg = n;
  int lane = threadIdx.x & 63;
  int wave = threadIdx.x >> 6;
  long long sm = (i < nseg) ? sums[i] : 0;
  int flag = sm != 0;
  uint64_t ball = __ballot(flag);
  __shared__ int wave_tot[PW_BLOCK / 64];
  if (lane == 0) wave_tot[wave] = __popcll(ball);
  __syncthreads();
  if (!WRITE) {
    if (threadIdx.x == 0) {
      int total = 0;
      for (int j = 0; j < PW_BLOCK / 64; ++j) total += wave_tot[j];
      block_counts[blockIdx.x] = total;
    }
  } else {
    int wave_base = 0;
    for (int j = 0; j < wave; ++j) wave_base += wave_tot[j];
    uint64_t below = ball & ((lane == 0) ? 0ULL : ((1ULL << lane) - 1));
    long long base = blockIdx.x ? block_csum[blockIdx.x - 1] : 0;
    long long pos = base + wave_base + __popcll(below);
    if (flag) {
      long long row = first[i];
      out_rows[pos] = row;
      out_w[pos] = sm;
      if (out_keys != nullptr) {
        out_keys[2 * pos] = keys[2 * row];
        out_keys[2 * pos + 1] = keys[2 * row + 1];
      }
    }
  }
}

// The whole consolidation on the caller's stream, no host read inside.
// keys (n,2) int64; column descriptors as pw_row_ident; diffs n int64.
// Scratch: ckeys (n,2) int64, temp (pw_gc_temp_bytes_prefix(n)), k0_sorted,
// k1_sorted, first, sums (n int64 each), perm32 (n uint32), dirty_list
// (max_dirty uint32), block_counts (ceil(n/256) int32), csum (ceil(n/256)
// int64).  Outputs: out_rows, out_w (n int64 each, ctl[2] of them valid),
// out_keys (null, or (n,2) int64: keys[out_rows[j]] in row j) and ctl
// (4 uint64, see above).  With ctl[0] set the outputs are void.
extern "C" int pw_consolidate_rows(
    const void* keys, int64_t n, const int* kinds, const void** a,
    const void** b, const void** c, const uint64_t* x, int ncols,
    uint64_t none_lo, uint64_t none_hi, const void* diffs, void* ckeys,
    void* temp, int64_t temp_bytes, void* k0_sorted, void* k1_sorted,
    void* perm32, int prefix_bits, int64_t max_run, int64_t max_dirty,
    void* dirty_list, void* ctl, void* block_counts, void* csum, void* first,
    void* sums, void* out_rows, void* out_w, void* out_keys, void* stream) {
  if (n < 2 || n >= ((int64_t)1 << 32)) return 1;
  RiCols cols;
  if (ri_fill(cols, kinds, a, b, c, x, ncols)) return 1;
  hipStream_t s = (hipStream_t)stream;
  int rc = ri_launch(keys, cols, ncols, none_lo, none_hi, n, ckeys, sums, s);
  if (rc) return rc;
  rc = pw_gc_prefix_sort_count(ckeys, n, temp, temp_bytes, k0_sorted,
                               k1_sorted, perm32, prefix_bits, max_run,
                               max_dirty, dirty_list, ctl, block_counts,
                               stream);
  if (rc) return rc;
  unsigned long long* ctlw = (unsigned long long*)ctl;
  int64_t nblocks = (n + PW_BLOCK - 1) / PW_BLOCK;
  dim3 grid((uint32_t)nblocks), block(PW_BLOCK);
  hipLaunchKernelGGL(k_cr_scan, dim3(1), dim3(PW_CR_SCAN_THREADS), 0, s,
                     (const int*)block_counts, nblocks, (long long*)csum,
                     ctlw + 3);
  hipLaunchKernelGGL(k_cr_emit, grid, block, 0, s,
                     (const long long*)k0_sorted, (const long long*)k1_sorted,
                     (const uint32_t*)perm32, (const long long*)diffs, n,
                     (const long long*)csum, (long long*)first,
                     (long long*)sums);
  hipLaunchKernelGGL((k_cr_nz<false>), grid, block, 0, s,
                     (const long long*)first, (const long long*)sums, n,
                     ctlw + 3, (int*)block_counts, (const long long*)csum,
                     (long long*)out_rows, (long long*)out_w,
                     (const long long*)keys, (long long*)out_keys);
  hipLaunchKernelGGL(k_cr_scan, dim3(1), dim3(PW_CR_SCAN_THREADS), 0, s,
                     (const int*)block_counts, nblocks, (long long*)csum,
                     ctlw + 2);
  hipLaunchKernelGGL((k_cr_nz<true>), grid, block, 0, s,
                     (const long long*)first, (const long long*)sums, n,
                     ctlw + 3, (int*)block_counts, (const long long*)csum,
                     (long long*)out_rows, (long long*)out_w,
                     (const long long*)keys, (long long*)out_keys);
  return (int)hipGetLastError();
}

// ------------------------------------------- multiset reducers: select --
//
// Segmented select behind min / max / argmin / argmax / earliest / latest /
// any: the multiset store keeps a group's rows contiguous, pw_key_range
// gives [lo, hi) per changed group, and these kernels pick one store row
// per range (-1 where no row of the range has a positive weight):
//
//   FIRST  the smallest row index of positive weight; no key is read
//   MIN    the smallest key, MAX the largest; equal keys go to the smallest
//          row index, as Python's min()/max() over the store order do
//
// int64 keys compare as int64.  float64 keys compare with < and >, so -0.0
// and 0.0 tie; a NaN beats every number in both modes and NaNs tie by row.
//
// k_seg_select_wave: one wave per range, lanes stride over the range, then
// a 64-lane __shfl_down reduction of the (key, row) pair; waves take ranges
// in a grid-stride loop.  A range longer than long_rows gets PW_SS_MARK and
// k_seg_select_long finishes it: a 1024-thread workgroup per marked range,
// a reduction per wave, then the 16 partials through LDS.  Every loop is
// bounded by hi - lo, bounds are clamped to the store, nothing is read back.

#define PW_SS_FIRST 0
#define PW_SS_MIN 1
#define PW_SS_MAX 2
#define PW_SS_MARK (-2LL)
#define PW_SS_LONG_THREADS 1024
#define PW_SS_LONG_GRID 1024

template <typename K>
__device__ __forceinline__ bool ss_isnan(K) {
  return false;
}
template <>
__device__ __forceinline__ bool ss_isnan<double>(double k) {
  return k != k;
}

// whether (ka, ra) is chosen over (kb, rb); a row of -1 is "none yet"
template <typename K, int MODE>
__device__ __forceinline__ bool ss_better(K ka, long long ra, K kb,
                                          long long rb) {
  if (ra < 0) return false;
  if (rb < 0) return true;
  if (MODE != PW_SS_FIRST) {
    const bool an = ss_isnan(ka), bn = ss_isnan(kb);
    if (an != bn) return an;
    if (!an) {
      if (MODE == PW_SS_MIN ? ka < kb : ka > kb) return true;
      if (MODE == PW_SS_MIN ? kb < ka : kb > ka) return false;
    }
  }
  return ra < rb;
}

template <typename K, int MODE>
__device__ __forceinline__ void ss_scan(const long long* __restrict__ weights,
                                        const K* __restrict__ key, int64_t lo,
                                        int64_t hi, int64_t start,
                                        int64_t step, K& bk, long long& br) {
  for (int64_t r = lo + start; r < hi; r += step) {
    if (weights[r] <= 0) continue;
    if (MODE == PW_SS_FIRST) {
      br = r;  // rows ascend: a lane's first positive row is its best
      break;
    }
    const K k = key[r];
    if (ss_better<K, MODE>(k, r, bk, br)) {
      bk = k;
      br = r;
    }
  }
}

// after this lane 0 holds the wave's best pair
template <typename K, int MODE>
__device__ __forceinline__ void ss_wave_reduce(K& bk, long long& br) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const K ok = __shfl_down(bk, off, 64);
    const long long orow = __shfl_down(br, off, 64);
    if (ss_better<K, MODE>(ok, orow, bk, br)) {
      bk = ok;
      br = orow;
    }
  }
}

__device__ __forceinline__ void ss_clamp(int64_t& lo, int64_t& hi, int64_t m) {
  if (lo < 0) lo = 0;
  if (hi > m) hi = m;
  if (hi < lo) hi = lo;
}

template <typename K, int MODE>
__global__ __launch_bounds__(PW_BLOCK) void k_seg_select_wave(
    const long long* __restrict__ lo_in, const long long* __restrict__ hi_in,
    int64_t nq, const long long* __restrict__ weights,
    const K* __restrict__ key, int64_t m, int64_t long_rows,
    long long* __restrict__ sel) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = ((int64_t)blockIdx.x * PW_BLOCK + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * PW_BLOCK) >> 6;
  for (int64_t q = wave; q < nq; q += nwaves) {
    int64_t lo = lo_in[q], hi = hi_in[q];
    ss_clamp(lo, hi, m);
    if (hi - lo > long_rows) {
      if (lane == 0) sel[q] = PW_SS_MARK;
      continue;
    }
    K bk = K(0);
    long long br = -1;
    ss_scan<K, MODE>(weights, key, lo, hi, lane, 64, bk, br);
    ss_wave_reduce<K, MODE>(bk, br);
    if (lane == 0) sel[q] = br;
  }
}

template <typename K, int MODE>
__global__ __launch_bounds__(PW_SS_LONG_THREADS) void k_seg_select_long(
    const long long* __restrict__ lo_in, const long long* __restrict__ hi_in,
    int64_t nq, const long long* __restrict__ weights,
    const K* __restrict__ key, int64_t m, long long* sel) {
  __shared__ K pk[PW_SS_LONG_THREADS / 64];
  __shared__ long long pr[PW_SS_LONG_THREADS / 64];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  for (int64_t q = blockIdx.x; q < nq; q += gridDim.x) {
    // every thread reads the marker before the barriers below, thread 0
    // overwrites it after them
    if (sel[q] != PW_SS_MARK) continue;
    int64_t lo = lo_in[q], hi = hi_in[q];
    ss_clamp(lo, hi, m);
    K bk = K(0);
    long long br = -1;
    ss_scan<K, MODE>(weights, key, lo, hi, tid, PW_SS_LONG_THREADS, bk, br);
    ss_wave_reduce<K, MODE>(bk, br);
    if (lane == 0) {
      pk[wv] = bk;
      pr[wv] = br;
    }
    __syncthreads();
    if (wv == 0) {
      const bool has = lane < PW_SS_LONG_THREADS / 64;
      bk = has ? pk[lane] : K(0);
      br = has ? pr[lane] : -1;
      ss_wave_reduce<K, MODE>(bk, br);
      if (lane == 0) sel[q] = br;
    }
    __syncthreads();
  }
}

template <typename K, int MODE>
static int ss_launch(const void* lo, const void* hi, int64_t nq,
                     const void* weights, const void* key, int64_t m,
                     int64_t long_rows, void* sel, hipStream_t s) {
  // four waves a block; the grid-stride loop takes the rest
  int64_t g = (nq + 3) / 4;
  if (g > PW_MAX_GRID) g = PW_MAX_GRID;
  hipLaunchKernelGGL((k_seg_select_wave<K, MODE>), dim3((uint32_t)g),
                     dim3(PW_BLOCK), 0, s, (const long long*)lo,
                     (const long long*)hi, nq, (const long long*)weights,
                     (const K*)key, m, long_rows, (long long*)sel);
  if (m > long_rows) {  // else no range can carry the marker
    int64_t gl = nq < PW_SS_LONG_GRID ? nq : PW_SS_LONG_GRID;
    hipLaunchKernelGGL((k_seg_select_long<K, MODE>), dim3((uint32_t)gl),
                       dim3(PW_SS_LONG_THREADS), 0, s, (const long long*)lo,
                       (const long long*)hi, nq, (const long long*)weights,
                       (const K*)key, m, (long long*)sel);
  }
  return (int)hipGetLastError();
}

// lo, hi, sel: nq int64; weights: m int64; key: m int64 (key_kind 1) or m
// float64 (key_kind 2), unused with mode FIRST; long_rows >= 64.
extern "C" int pw_seg_select(const void* lo, const void* hi, int64_t nq,
                             const void* weights, const void* key,
                             int key_kind, int64_t m, int mode,
                             int64_t long_rows, void* sel, void* stream) {
  if (nq < 0 || m < 0 || long_rows < 64) return 1;
  if (nq == 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  if (mode == PW_SS_FIRST)
    return ss_launch<long long, PW_SS_FIRST>(lo, hi, nq, weights, nullptr, m,
                                             long_rows, sel, s);
  if (mode != PW_SS_MIN && mode != PW_SS_MAX) return 1;
  if (key == nullptr && m > 0) return 1;
  const bool mn = mode == PW_SS_MIN;
  if (key_kind == 1)
    return mn ? ss_launch<long long, PW_SS_MIN>(lo, hi, nq, weights, key, m,
                                                long_rows, sel, s)
              : ss_launch<long long, PW_SS_MAX>(lo, hi, nq, weights, key, m,
                                                long_rows, sel, s);
  if (key_kind == 2)
    return mn ? ss_launch<double, PW_SS_MIN>(lo, hi, nq, weights, key, m,
                                             long_rows, sel, s)
              : ss_launch<double, PW_SS_MAX>(lo, hi, nq, weights, key, m,
                                             long_rows, sel, s);
  return 1;
}

// ----------------------------------------- multiset reducers: distinct --
//
// Number of distinct 64-bit values among the rows of positive weight of
// every range (count_distinct, and unique through count == 1), with the
// range's first such row.  One workgroup per range, ranges in a grid-stride
// loop.  The set is an open-addressing table of row offsets in LDS, in the
// idiom of k_gc_bucket_agg: a slot is claimed by a CAS of the row's offset
// over EMPTY, and a slot's value is read from the row that owns it, so no
// value needs a sentinel and no thread waits on another.
//
// One pass may claim max_hold slots (the table at its load limit).  A range
// with more distinct values than that is counted in P passes, P a power of
// two: pass p inserts the values whose mixed hash has p in its top bits,
// the slot comes from the low bits, and the table is cleared between
// passes.  P is found by doubling: the count starts at one pass, and a pass
// that would claim slot max_hold + 1 ends the attempt at once and starts
// the next with 2 P, so a long range of few values costs one pass and the
// attempts that fail cost about max_hold claims each.  A range that
// overflows a pass at PW_SD_MAX_PASSES passes (any range of more than
// PW_SD_MAX_PASSES * max_hold distinct values does), or an insert that runs
// out of max_probe probes, gives the range up: status 1, count 0, first -1.

#define PW_SD_THREADS 1024
#define PW_SD_GRID 1024
#define PW_SD_EMPTY 0xFFFFFFFFu
#define PW_SD_MAX_PASSES 64
#define PW_SD_MAX_CAPACITY 8192  // 32 KB of LDS

__device__ __forceinline__ uint64_t sd_mix(uint64_t x) {
  x ^= x >> 33;
  x *= 0xFF51AFD7ED558CCDULL;
  x ^= x >> 33;
  x *= 0xC4CEB9FE1A85EC53ULL;
  x ^= x >> 33;
  return x;
}

__global__ __launch_bounds__(PW_SD_THREADS) void k_seg_distinct(
    const long long* __restrict__ lo_in, const long long* __restrict__ hi_in,
    int64_t nq, const long long* __restrict__ weights,
    const long long* __restrict__ values, int64_t m, uint32_t cap,
    uint32_t max_hold, uint32_t max_probe, long long* __restrict__ count,
    long long* __restrict__ first, int* __restrict__ status) {
  extern __shared__ uint32_t sd_tab[];  // [cap] row offsets into the range
  // s_stop: 1 = a pass is over its share (next attempt), 2 = out of probes
  __shared__ uint32_t s_claims, s_first, s_stop;
  const uint32_t tid = threadIdx.x;
  for (int64_t q = blockIdx.x; q < nq; q += gridDim.x) {
    int64_t lo = lo_in[q], hi = hi_in[q];
    ss_clamp(lo, hi, m);
    const int64_t len = hi - lo;
    if (len >= (int64_t)PW_SD_EMPTY) {  // offsets are 32 bits; uniform
      if (tid == 0) count[q] = 0, first[q] = -1, status[q] = 1;
      continue;
    }
    const uint32_t rows = (uint32_t)len;
    // a short range clears and probes only the table it needs
    uint32_t tcap = cap;
    if (rows <= max_hold) {
      tcap = 64;
      while (tcap < 2 * rows && tcap < cap) tcap <<= 1;
    }
    const uint32_t mask = tcap - 1;
    const uint32_t probes = max_probe < tcap ? max_probe : tcap;
    if (tid == 0) s_first = PW_SD_EMPTY;
    uint32_t myfirst = PW_SD_EMPTY;
    uint32_t total = 0, stop = 0;
    int lg_passes = 0;
    for (;;) {  // attempts: 1, 2, 4, ... PW_SD_MAX_PASSES passes
      total = 0;
      for (uint32_t p = 0; p < (1u << lg_passes); ++p) {
        if (tid == 0) s_claims = 0, s_stop = 0;
        for (uint32_t sl = tid; sl < tcap; sl += PW_SD_THREADS)
          sd_tab[sl] = PW_SD_EMPTY;
        __syncthreads();
        for (uint32_t i = tid; i < rows; i += PW_SD_THREADS) {
          if (__hip_atomic_load(&s_stop, __ATOMIC_RELAXED,
                                __HIP_MEMORY_SCOPE_WORKGROUP))
            break;
          if (weights[lo + i] <= 0) continue;
          if (i < myfirst) myfirst = i;
          const long long v = values[lo + i];
          const uint64_t h = sd_mix((uint64_t)v);
          if (lg_passes && (uint32_t)(h >> (64 - lg_passes)) != p) continue;
          uint32_t slot = (uint32_t)h & mask;
          bool done = false;
          for (uint32_t t = 0; t < probes; ++t) {
            uint32_t cur = __hip_atomic_load(&sd_tab[slot], __ATOMIC_RELAXED,
                                             __HIP_MEMORY_SCOPE_WORKGROUP);
            if (cur == PW_SD_EMPTY) {
              cur = atomicCAS(&sd_tab[slot], PW_SD_EMPTY, i);
              if (cur == PW_SD_EMPTY) {  // claimed: a new value
                if (atomicAdd(&s_claims, 1u) >= max_hold) atomicMax(&s_stop, 1u);
                done = true;
                break;
              }
            }
            if (values[lo + cur] == v) {  // cur < rows: some row's own offset
              done = true;
              break;
            }
            slot = (slot + 1) & mask;
          }
          if (!done) atomicMax(&s_stop, 2u);
        }
        __syncthreads();
        stop = s_stop;
        total += s_claims;
        __syncthreads();  // all have read before thread 0 resets
        if (stop) break;
      }
      if (stop != 1 || (1 << lg_passes) >= PW_SD_MAX_PASSES) break;
      ++lg_passes;
    }
    // the attempt that held visited every row in its pass 0
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const uint32_t of = __shfl_down(myfirst, off, 64);
      myfirst = of < myfirst ? of : myfirst;
    }
    if ((tid & 63) == 0 && myfirst != PW_SD_EMPTY) atomicMin(&s_first, myfirst);
    __syncthreads();
    if (tid == 0) {
      const bool ok = stop == 0 && s_first != PW_SD_EMPTY;
      count[q] = stop ? 0 : (long long)total;
      first[q] = ok ? lo + (int64_t)s_first : -1;
      status[q] = stop ? 1 : 0;
    }
    __syncthreads();
  }
}

// lo, hi, count, first: nq int64; status: nq int32; weights, values: m
// int64.  table_capacity: a power of two in [64, PW_SD_MAX_CAPACITY];
// max_hold in [1, table_capacity): rows one pass is sized for.
extern "C" int pw_seg_distinct(const void* lo, const void* hi, int64_t nq,
                               const void* weights, const void* values,
                               int64_t m, int64_t table_capacity,
                               int64_t max_hold, int64_t max_probe,
                               void* count, void* first, void* status,
                               void* stream) {
  if (nq < 0 || m < 0) return 1;
  if (table_capacity < 64 || table_capacity > PW_SD_MAX_CAPACITY ||
      (table_capacity & (table_capacity - 1)))
    return 1;
  if (max_hold < 1 || max_hold >= table_capacity || max_probe < 1) return 1;
  if (nq == 0) return 0;
  if (max_probe > table_capacity) max_probe = table_capacity;
  int64_t g = nq < PW_SD_GRID ? nq : PW_SD_GRID;
  hipLaunchKernelGGL(k_seg_distinct, dim3((uint32_t)g), dim3(PW_SD_THREADS),
                     (size_t)table_capacity * sizeof(uint32_t),
                     (hipStream_t)stream, (const long long*)lo,
                     (const long long*)hi, nq, (const long long*)weights,
                     (const long long*)values, m, (uint32_t)table_capacity,
                     (uint32_t)max_hold, (uint32_t)max_probe,
                     (long long*)count, (long long*)first, (int*)status);
  return (int)hipGetLastError();
}

// ------------------------------------------- segmented double-double sum --
// Float sums of the group reduce: per segment of a permuted batch, the sum
// of up to 8 float64 columns as a double-double (hi, lo) pair, without
// float atomics.  The value of a segment is a function of its values in
// permuted order and of its length alone, so that the same rows give the
// same bits wherever they sit in the batch and whatever the grid:
//
//   L <= T   W(v[0..L)): lane l of a wave adds v[l], v[l+64], ... in order,
//            then six butterfly steps (xor 1, 2, 4, 8, 16, 32) add the
//            lanes; lane 0 holds the result.  For L <= 8 eight segments
//            share a wave, one per aligned group of 8 lanes with three
//            butterfly steps: the same sums, since the lanes that are
//            left out would add (0, 0), which is exact.
//   L >  T   the segment is listed and cut into chunks of T rows counted
//            from its start.  k_ssf_chunk reduces one chunk per workgroup
//            (thread t adds v[t], v[t+256], ...; butterfly per wave; the
//            four wave results added in wave order) into a scratch slot;
//            k_ssf_combine applies W to the segment's chunk results in
//            chunk order.
//
// k_ssf_short takes 8 consecutive segments per wave: the short ones in
// 8-lane groups at once, the others up to T one after another with the
// whole wave, and lists the long ones (integer atomics reserve list entries
// and chunk slots; in which order does not reach the result).  No host
// read: list and slots are sized by n / T, the later kernels are launched
// for that many and leave at once where nothing was listed.
//
// The step is Knuth's TwoSum of the high parts, the low parts added to
// its error term, and a renormalisation: adds and subtracts only, so no
// contraction to FMA can change it.  A sum whose high part stops being
// finite is that high part with a low part of 0, as plain float64
// addition would give (inf stays inf, inf - inf and NaN are NaN).

struct PwDD {
  double h, l;
};

__device__ __forceinline__ PwDD pw_dd_add(PwDD a, PwDD b) {
  double s = a.h + b.h;
  if (!isfinite(s)) return PwDD{s, 0.0};
  double bb = s - a.h;
  double e = (a.h - (s - bb)) + (b.h - bb);
  e += a.l + b.l;
  double h = s + e;
  if (!isfinite(h)) return PwDD{h, 0.0};
  return PwDD{h, e - (h - s)};
}

__device__ __forceinline__ PwDD pw_dd_xor(PwDD a, int mask) {
  return PwDD{__shfl_xor(a.h, mask, 64), __shfl_xor(a.l, mask, 64)};
}

// own value first, so that lane 0 adds in the order the comment gives
template <int STEPS>
__device__ __forceinline__ PwDD pw_dd_butterfly(PwDD a) {
#pragma unroll
  for (int k = 0; k < STEPS; ++k) a = pw_dd_add(a, pw_dd_xor(a, 1 << k));
  return a;
}

struct F64Ptrs {
  const double* p[8];
};
struct F64PtrsMut {
  double* p[8];
};

// PM: 0 identity, 1 uint32 permutation, 2 int64 permutation.  A row
// outside [0, n) reads as NaN instead of out of bounds.
template <int PM>
__device__ __forceinline__ PwDD ssf_load(const void* perm, const double* hi,
                                         const double* lo, int64_t i,
                                         int64_t n) {
  int64_t row = PM == 0   ? i
                : PM == 1 ? (int64_t)((const uint32_t*)perm)[i]
                          : (int64_t)((const long long*)perm)[i];
  if ((uint64_t)row >= (uint64_t)n)
    return PwDD{__longlong_as_double(0x7ff8000000000000LL), 0.0};
  return PwDD{hi[row], lo ? lo[row] : 0.0};
}

__device__ __forceinline__ int64_t ssf_clamp(long long v, int64_t n) {
  return v < 0 ? 0 : (v > n ? n : (int64_t)v);
}

#define PW_SSF_SHORT 8  // segments per wave = lanes per short segment

// ctl[0]: listed segments, ctl[1]: chunk slots taken (zeroed by the caller)
// list: (seg, first slot, chunks) per entry; desc: (seg, chunk) per slot
template <int PM>
__global__ void k_ssf_short(const void* perm,
                            const long long* __restrict__ seg_start,
                            int64_t nseg, int64_t n, F64Ptrs hi, F64Ptrs lo,
                            int ncol, int64_t T, F64PtrsMut out_hi,
                            F64PtrsMut out_lo, unsigned long long* ctl,
                            long long* list, long long* desc,
                            int64_t max_list, int64_t max_slots) {
  int lane = threadIdx.x & 63;
  int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  int g = lane >> 3, j = lane & 7;
  int64_t s = wave * PW_SSF_SHORT + g;
  int64_t b = 0, L = -1;  // L < 0: no segment
  if (s < nseg) {
    b = ssf_clamp(seg_start[s], n);
    int64_t e = ssf_clamp(seg_start[s + 1], n);
    L = e > b ? e - b : 0;
  }
  const PwDD zero{0.0, 0.0};
  // short segments, one per 8-lane group
  bool is_short = L >= 0 && L <= PW_SSF_SHORT;
  if (__ballot(is_short)) {
    for (int c = 0; c < ncol; ++c) {
      PwDD v = zero;
      if (is_short && j < L)
        v = pw_dd_add(zero, ssf_load<PM>(perm, hi.p[c], lo.p[c], b + j, n));
      v = pw_dd_butterfly<3>(v);
      if (is_short && j == 0) {
        out_hi.p[c][s] = v.h;
        out_lo.p[c][s] = v.l;
      }
    }
  }
  // the others up to T, one after another with the whole wave
  uint64_t mid = __ballot(j == 0 && L > PW_SSF_SHORT && L <= T);
  while (mid) {
    int src = __ffsll((unsigned long long)mid) - 1;
    mid &= mid - 1;
    int64_t sb = __shfl(b, src, 64), sL = __shfl(L, src, 64);
    int64_t ss = wave * PW_SSF_SHORT + (src >> 3);
    for (int c = 0; c < ncol; ++c) {
      PwDD acc = zero;
#pragma unroll 4
      for (int64_t i = lane; i < sL; i += 64)
        acc = pw_dd_add(acc, ssf_load<PM>(perm, hi.p[c], lo.p[c], sb + i, n));
      acc = pw_dd_butterfly<6>(acc);
      if (lane == 0) {
        out_hi.p[c][ss] = acc.h;
        out_lo.p[c][ss] = acc.l;
      }
    }
  }
  // long segments: list them and hand out their chunk slots
  uint64_t lng = __ballot(j == 0 && L > T);
  while (lng) {
    int src = __ffsll((unsigned long long)lng) - 1;
    lng &= lng - 1;
    int64_t sL = __shfl(L, src, 64);
    int64_t ss = wave * PW_SSF_SHORT + (src >> 3);
    int64_t nch = (sL + T - 1) / T;
    long long idx = 0, base = 0;
    if (lane == 0) {
      idx = (long long)atomicAdd(&ctl[0], 1ULL);
      base = (long long)atomicAdd(&ctl[1], (unsigned long long)nch);
    }
    idx = __shfl(idx, 0, 64);
    base = __shfl(base, 0, 64);
    // cannot happen for ascending seg_start within [0, n]
    bool fits = idx < max_list && base + nch <= max_slots;
    if (lane == 0 && idx < max_list) {
      list[3 * idx] = ss;
      list[3 * idx + 1] = base;
      list[3 * idx + 2] = fits ? nch : -1;
    }
    if (fits) {
      for (int64_t k = lane; k < nch; k += 64) {
        desc[2 * (base + k)] = ss;
        desc[2 * (base + k) + 1] = k;
      }
    } else if (lane == 0 && idx >= max_list) {
      for (int c = 0; c < ncol; ++c) {
        out_hi.p[c][ss] = __longlong_as_double(0x7ff8000000000000LL);
        out_lo.p[c][ss] = 0.0;
      }
    }
  }
}

// parts: (2 * ncol, max_slots) doubles: hi and lo row of every column
template <int PM>
__global__ void k_ssf_chunk(const void* perm,
                            const long long* __restrict__ seg_start,
                            int64_t nseg, int64_t n, F64Ptrs hi, F64Ptrs lo,
                            int ncol, int64_t T,
                            const unsigned long long* __restrict__ ctl,
                            const long long* __restrict__ desc, double* parts,
                            int64_t max_slots) {
  int64_t slot = blockIdx.x;
  unsigned long long taken = ctl[1];
  if (slot >= max_slots || (unsigned long long)slot >= taken) return;
  int64_t s = desc[2 * slot], k = desc[2 * slot + 1];
  if (s < 0 || s >= nseg || k < 0 || k > n / T) return;
  int64_t b0 = ssf_clamp(seg_start[s], n), e0 = ssf_clamp(seg_start[s + 1], n);
  int64_t b = b0 + k * T;
  int64_t e = b + T < e0 ? b + T : e0;
  int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  __shared__ PwDD wave_sum[PW_BLOCK / 64];
  const PwDD zero{0.0, 0.0};
  for (int c = 0; c < ncol; ++c) {
    PwDD acc = zero;
#pragma unroll 4
    for (int64_t i = b + threadIdx.x; i < e; i += PW_BLOCK)
      acc = pw_dd_add(acc, ssf_load<PM>(perm, hi.p[c], lo.p[c], i, n));
    acc = pw_dd_butterfly<6>(acc);
    if (lane == 0) wave_sum[wv] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
      PwDD r = wave_sum[0];
      for (int w = 1; w < PW_BLOCK / 64; ++w) r = pw_dd_add(r, wave_sum[w]);
      parts[(size_t)(2 * c) * max_slots + slot] = r.h;
      parts[(size_t)(2 * c + 1) * max_slots + slot] = r.l;
    }
    __syncthreads();
  }
}

__global__ void k_ssf_combine(int64_t nseg, int ncol,
                              const unsigned long long* __restrict__ ctl,
                              const long long* __restrict__ list,
                              const double* __restrict__ parts,
                              int64_t max_list, int64_t max_slots,
                              F64PtrsMut out_hi, F64PtrsMut out_lo) {
  int lane = threadIdx.x & 63;
  int64_t idx = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  unsigned long long listed = ctl[0];
  if (idx >= max_list || (unsigned long long)idx >= listed) return;
  int64_t s = list[3 * idx], base = list[3 * idx + 1], nch = list[3 * idx + 2];
  if (s < 0 || s >= nseg) return;
  const PwDD zero{0.0, 0.0};
  for (int c = 0; c < ncol; ++c) {
    PwDD acc = zero;
    if (nch < 0) acc.h = __longlong_as_double(0x7ff8000000000000LL);
    const double* ph = parts + (size_t)(2 * c) * max_slots + base;
    const double* pl = parts + (size_t)(2 * c + 1) * max_slots + base;
    for (int64_t k = lane; k < nch; k += 64)
      acc = pw_dd_add(acc, PwDD{ph[k], pl[k]});
    acc = pw_dd_butterfly<6>(acc);
    if (lane == 0) {
      out_hi.p[c][s] = acc.h;
      out_lo.p[c][s] = acc.l;
    }
  }
}

template <int PM>
static void ssf_launch(const void* perm, const long long* seg_start,
                       int64_t nseg, int64_t n, F64Ptrs hp, F64Ptrs lp,
                       int ncol, int64_t T, F64PtrsMut oh, F64PtrsMut ol,
                       unsigned long long* ctl, long long* list,
                       long long* desc, double* parts, int64_t max_list,
                       int64_t max_slots, hipStream_t s) {
  int64_t waves = (nseg + PW_SSF_SHORT - 1) / PW_SSF_SHORT;
  int64_t blocks = (waves * 64 + PW_BLOCK - 1) / PW_BLOCK;
  hipLaunchKernelGGL(k_ssf_short<PM>, dim3((uint32_t)blocks), dim3(PW_BLOCK),
                     0, s, perm, seg_start, nseg, n, hp, lp, ncol, T, oh, ol,
                     ctl, list, desc, max_list, max_slots);
  if (n <= T) return;  // no segment can be long
  hipLaunchKernelGGL(k_ssf_chunk<PM>, dim3((uint32_t)max_slots),
                     dim3(PW_BLOCK), 0, s, perm, seg_start, nseg, n, hp, lp,
                     ncol, T, ctl, desc, parts, max_slots);
  int64_t cblocks = (max_list * 64 + PW_BLOCK - 1) / PW_BLOCK;
  hipLaunchKernelGGL(k_ssf_combine, dim3((uint32_t)cblocks), dim3(PW_BLOCK), 0,
                     s, nseg, ncol, ctl, list, parts, max_list, max_slots, oh,
                     ol);
}

// perm: n row indices (perm_mode 1: uint32, 2: int64) or unused (0:
// identity).  seg_start: nseg + 1 int64, ascending, from 0 to n.  hi_ptrs:
// ncol float64 columns of n; lo_ptrs: null, or their low parts.  out_hi,
// out_lo: ncol columns of nseg.  ctl: 2 uint64, ZEROED by the caller.
// list: 3 * max_list int64, desc: 2 * max_slots int64, parts: 2 * ncol *
// max_slots float64, with max_list >= n / T + 1 and max_slots >= n / T +
// max_list (a long segment of L rows takes ceil(L / T) < L / T + 1 slots).
extern "C" int pw_seg_sum_f64(const void* perm, int perm_mode,
                              const void* seg_start, int64_t nseg, int64_t n,
                              const void** hi_ptrs, const void** lo_ptrs,
                              int ncol, int64_t T, void** out_hi,
                              void** out_lo, void* ctl, void* list, void* desc,
                              void* parts, int64_t max_list, int64_t max_slots,
                              void* stream) {
  if (ncol < 1 || ncol > 8 || nseg < 0 || n < 0) return 1;
  if (perm_mode < 0 || perm_mode > 2 || (perm_mode && !perm)) return 1;
  if (T < 64 || T > ((int64_t)1 << 24)) return 1;
  if (max_list < n / T + 1 || max_slots < n / T + max_list) return 1;
  if (max_slots >= ((int64_t)1 << 31)) return 1;
  if (nseg == 0) return 0;
  F64Ptrs hp, lp;
  F64PtrsMut oh, ol;
  for (int c = 0; c < 8; ++c) {
    hp.p[c] = c < ncol ? (const double*)hi_ptrs[c] : nullptr;
    lp.p[c] = (c < ncol && lo_ptrs) ? (const double*)lo_ptrs[c] : nullptr;
    oh.p[c] = c < ncol ? (double*)out_hi[c] : nullptr;
    ol.p[c] = c < ncol ? (double*)out_lo[c] : nullptr;
  }
  hipStream_t s = (hipStream_t)stream;
  if (perm_mode == 0)
    ssf_launch<0>(perm, (const long long*)seg_start, nseg, n, hp, lp, ncol, T,
                  oh, ol, (unsigned long long*)ctl, (long long*)list,
                  (long long*)desc, (double*)parts, max_list, max_slots, s);
  else if (perm_mode == 1)
    ssf_launch<1>(perm, (const long long*)seg_start, nseg, n, hp, lp, ncol, T,
                  oh, ol, (unsigned long long*)ctl, (long long*)list,
                  (long long*)desc, (double*)parts, max_list, max_slots, s);
  else
    ssf_launch<2>(perm, (const long long*)seg_start, nseg, n, hp, lp, ncol, T,
                  oh, ol, (unsigned long long*)ctl, (long long*)list,
                  (long long*)desc, (double*)parts, max_list, max_slots, s);
  return (int)hipGetLastError();
}
