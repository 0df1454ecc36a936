// Shared xxh64 primitives — compiled for HOST (pool hashing, static tables)
// and DEVICE (batch key hashing on gfx950) from the same source so keys are
// bit-identical everywhere.  Mirrors pathway_amd/internals/api.py:xxh64 and
// the torch reference pathway_amd/engine/hashing.py (tests/test_hash.py
// checks all three agree).
//
// Reference semantics: 128-bit key = xxh64(seed=SEED_LO) || xxh64(seed=SEED_HI)
// over the canonical tagged serialization (value.rs:40-66 analog).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define PW_HD __host__ __device__ __forceinline__
#else
#define PW_HD static inline
#endif

#define PW_P1 0x9E3779B185EBCA87ULL
#define PW_P2 0xC2B2AE3D27D4EB4FULL
#define PW_P3 0x165667B19E3779F9ULL
#define PW_P4 0x85EBCA77C2B2AE63ULL
#define PW_P5 0x27D4EB2F165667C5ULL

#define PW_SEED_LO 0ULL
#define PW_SEED_HI 0x9E3779B185EBCA87ULL

PW_HD uint64_t pw_rotl64(uint64_t x, int r) { return (x << r) | (x >> (64 - r)); }

PW_HD uint64_t pw_round(uint64_t acc, uint64_t inp) {
  acc += inp * PW_P2;
  acc = pw_rotl64(acc, 31);
  return acc * PW_P1;
}

PW_HD uint64_t pw_merge_round(uint64_t acc, uint64_t val) {
  val = pw_round(0, val);
  acc ^= val;
  return acc * PW_P1 + PW_P4;
}

PW_HD uint64_t pw_avalanche(uint64_t h) {
  h ^= h >> 33;
  h *= PW_P2;
  h ^= h >> 29;
  h *= PW_P3;
  h ^= h >> 32;
  return h;
}

// xxh64 over W little-endian 8-byte words held in a local array.
template <int W>
PW_HD uint64_t pw_xxh64_words(const uint64_t* w, uint64_t seed) {
  const int nbytes = W * 8;
  uint64_t h;
  int i = 0;
  if (nbytes >= 32) {
    uint64_t v1 = seed + PW_P1 + PW_P2;
    uint64_t v2 = seed + PW_P2;
    uint64_t v3 = seed;
    uint64_t v4 = seed - PW_P1;
    while (i + 4 <= W) {
      v1 = pw_round(v1, w[i]);
      v2 = pw_round(v2, w[i + 1]);
      v3 = pw_round(v3, w[i + 2]);
      v4 = pw_round(v4, w[i + 3]);
      i += 4;
    }
    h = pw_rotl64(v1, 1) + pw_rotl64(v2, 7) + pw_rotl64(v3, 12) + pw_rotl64(v4, 18);
    h = pw_merge_round(h, v1);
    h = pw_merge_round(h, v2);
    h = pw_merge_round(h, v3);
    h = pw_merge_round(h, v4);
  } else {
    h = seed + PW_P5;
  }
  h += (uint64_t)nbytes;
  for (; i < W; ++i) {
    h ^= pw_round(0, w[i]);
    h = pw_rotl64(h, 27) * PW_P1 + PW_P4;
  }
  return pw_avalanche(h);
}

// general byte-range xxh64 (for varlen string/bytes hashing)
PW_HD uint64_t pw_xxh64_bytes(const uint8_t* data, int64_t n, uint64_t seed) {
  int64_t i = 0;
  uint64_t h;
  if (n >= 32) {
    uint64_t v1 = seed + PW_P1 + PW_P2;
    uint64_t v2 = seed + PW_P2;
    uint64_t v3 = seed;
    uint64_t v4 = seed - PW_P1;
    while (i + 32 <= n) {
      uint64_t a, b, c, d;
      __builtin_memcpy(&a, data + i, 8);
      __builtin_memcpy(&b, data + i + 8, 8);
      __builtin_memcpy(&c, data + i + 16, 8);
      __builtin_memcpy(&d, data + i + 24, 8);
      v1 = pw_round(v1, a);
      v2 = pw_round(v2, b);
      v3 = pw_round(v3, c);
      v4 = pw_round(v4, d);
      i += 32;
    }
    h = pw_rotl64(v1, 1) + pw_rotl64(v2, 7) + pw_rotl64(v3, 12) + pw_rotl64(v4, 18);
    h = pw_merge_round(h, v1);
    h = pw_merge_round(h, v2);
    h = pw_merge_round(h, v3);
    h = pw_merge_round(h, v4);
  } else {
    h = seed + PW_P5;
  }
  h += (uint64_t)n;
  while (i + 8 <= n) {
    uint64_t k;
    __builtin_memcpy(&k, data + i, 8);
    h ^= pw_round(0, k);
    h = pw_rotl64(h, 27) * PW_P1 + PW_P4;
    i += 8;
  }
  while (i + 4 <= n) {
    uint32_t k;
    __builtin_memcpy(&k, data + i, 4);
    h ^= (uint64_t)k * PW_P1;
    h = pw_rotl64(h, 23) * PW_P2 + PW_P3;
    i += 4;
  }
  while (i < n) {
    h ^= (uint64_t)data[i] * PW_P5;
    h = pw_rotl64(h, 11) * PW_P1;
    i += 1;
  }
  return pw_avalanche(h);
}

// ---- tagged token hash, both seeds in one walk ---------------------------
//
// pw_xxh64_tagged2: the two 64-bit hashes (PW_SEED_LO, PW_SEED_HI) of the
// message  tag (8 bytes LE) || base[a : a+len]  for any len >= 0, equal to
// pw_xxh64_bytes over the concatenation.  The data is walked once: every
// word is loaded once and fed to both seeds' states.  Nothing is staged and
// no array is indexed at run time, so on the device everything stays in
// registers.
//
// Data words come from aligned 4-byte loads at the token's address rounded
// down to a multiple of 4, combined with shifts (neighbouring lanes read
// neighbouring or the same dwords).  No load touches a byte outside
// [base, base + nbytes): a dword that would begin before base or end after
// base + nbytes is put together from its in-range bytes, and a dword that
// holds no byte of the token is not loaded at all.  base needs no alignment.

// the aligned dword at address q (q % 4 == 0), for a token ending at tend
// inside the buffer [blo, bhi)
PW_HD uint32_t pw_tok_dword(uintptr_t q, uintptr_t tend, uintptr_t blo,
                            uintptr_t bhi) {
  if (q >= tend) return 0;  // no byte of the token in it
  if (q >= blo && q + 4 <= bhi) {
    uint32_t v;
    __builtin_memcpy(&v, __builtin_assume_aligned((const void*)q, 4), 4);
    return v;
  }
  uint32_t v = 0;
  if (q + 0 >= blo && q + 0 < bhi) v |= (uint32_t)(*(const uint8_t*)(q + 0));
  if (q + 1 >= blo && q + 1 < bhi) v |= (uint32_t)(*(const uint8_t*)(q + 1)) << 8;
  if (q + 2 >= blo && q + 2 < bhi) v |= (uint32_t)(*(const uint8_t*)(q + 2)) << 16;
  if (q + 3 >= blo && q + 3 < bhi) v |= (uint32_t)(*(const uint8_t*)(q + 3)) << 24;
  return v;
}

// Sequential reader of a token's bytes, 4 at a time, from aligned dwords.
struct PwTokReader {
  uintptr_t q;     // address of the next aligned dword
  uintptr_t tend;  // one past the token's last byte
  uintptr_t blo, bhi;
  uint32_t carry;  // the dword before q
  int sh;          // bit offset of the token's next byte inside carry
};

PW_HD void pw_tok_open(PwTokReader* r, const uint8_t* base, int64_t nbytes,
                       int64_t a, int64_t len) {
  const uintptr_t p = (uintptr_t)base + (uintptr_t)a;
  r->blo = (uintptr_t)base;
  r->bhi = (uintptr_t)base + (uintptr_t)nbytes;
  r->tend = p + (uintptr_t)(len > 0 ? len : 0);
  r->sh = (int)(p & 3) * 8;
  r->q = p & ~(uintptr_t)3;
  r->carry = pw_tok_dword(r->q, r->tend, r->blo, r->bhi);
  r->q += 4;
}

// The token's next 4 bytes, little-endian.  Bytes past the token's end are
// NOT zero: the dword that holds its last byte also carries the buffer's
// bytes behind it, so a caller uses only as many bytes as the token has left.
PW_HD uint32_t pw_tok_next32(PwTokReader* r) {
  const uint32_t d = pw_tok_dword(r->q, r->tend, r->blo, r->bhi);
  const uint32_t v = (uint32_t)((((uint64_t)d << 32) | r->carry) >> r->sh);
  r->carry = d;
  r->q += 4;
  return v;
}

PW_HD uint64_t pw_tok_next64(PwTokReader* r) {
  const uint64_t lo = pw_tok_next32(r);
  const uint64_t hi = pw_tok_next32(r);
  return lo | (hi << 32);
}

struct PwHash128 {
  uint64_t lo, hi;
};

PW_HD PwHash128 pw_xxh64_tagged2(const uint8_t* base, int64_t nbytes,
                                 int64_t a, int64_t len, uint64_t tag) {
  if (len < 0) len = 0;
  PwTokReader r;
  pw_tok_open(&r, base, nbytes, a, len);
  int64_t rem = len;  // token bytes not yet consumed
  uint64_t h0, h1;
  if (len + 8 >= 32) {
    uint64_t a1 = PW_SEED_LO + PW_P1 + PW_P2, b1 = PW_SEED_HI + PW_P1 + PW_P2;
    uint64_t a2 = PW_SEED_LO + PW_P2, b2 = PW_SEED_HI + PW_P2;
    uint64_t a3 = PW_SEED_LO, b3 = PW_SEED_HI;
    uint64_t a4 = PW_SEED_LO - PW_P1, b4 = PW_SEED_HI - PW_P1;
    // first stripe: the tag word and the first 24 token bytes
    uint64_t w = tag;
    a1 = pw_round(a1, w), b1 = pw_round(b1, w);
    w = pw_tok_next64(&r);
    a2 = pw_round(a2, w), b2 = pw_round(b2, w);
    w = pw_tok_next64(&r);
    a3 = pw_round(a3, w), b3 = pw_round(b3, w);
    w = pw_tok_next64(&r);
    a4 = pw_round(a4, w), b4 = pw_round(b4, w);
    rem -= 24;
    while (rem >= 32) {
      w = pw_tok_next64(&r);
      a1 = pw_round(a1, w), b1 = pw_round(b1, w);
      w = pw_tok_next64(&r);
      a2 = pw_round(a2, w), b2 = pw_round(b2, w);
      w = pw_tok_next64(&r);
      a3 = pw_round(a3, w), b3 = pw_round(b3, w);
      w = pw_tok_next64(&r);
      a4 = pw_round(a4, w), b4 = pw_round(b4, w);
      rem -= 32;
    }
    h0 = pw_rotl64(a1, 1) + pw_rotl64(a2, 7) + pw_rotl64(a3, 12) + pw_rotl64(a4, 18);
    h0 = pw_merge_round(h0, a1);
    h0 = pw_merge_round(h0, a2);
    h0 = pw_merge_round(h0, a3);
    h0 = pw_merge_round(h0, a4);
    h1 = pw_rotl64(b1, 1) + pw_rotl64(b2, 7) + pw_rotl64(b3, 12) + pw_rotl64(b4, 18);
    h1 = pw_merge_round(h1, b1);
    h1 = pw_merge_round(h1, b2);
    h1 = pw_merge_round(h1, b3);
    h1 = pw_merge_round(h1, b4);
    h0 += (uint64_t)(len + 8);
    h1 += (uint64_t)(len + 8);
  } else {
    // no stripe: the tag is the first 8-byte step of the tail
    h0 = PW_SEED_LO + PW_P5 + (uint64_t)(len + 8);
    h1 = PW_SEED_HI + PW_P5 + (uint64_t)(len + 8);
    const uint64_t k = pw_round(0, tag);
    h0 = pw_rotl64(h0 ^ k, 27) * PW_P1 + PW_P4;
    h1 = pw_rotl64(h1 ^ k, 27) * PW_P1 + PW_P4;
  }
  while (rem >= 8) {
    const uint64_t k = pw_round(0, pw_tok_next64(&r));
    h0 = pw_rotl64(h0 ^ k, 27) * PW_P1 + PW_P4;
    h1 = pw_rotl64(h1 ^ k, 27) * PW_P1 + PW_P4;
    rem -= 8;
  }
  if (rem >= 4) {
    const uint64_t k = (uint64_t)pw_tok_next32(&r) * PW_P1;
    h0 = pw_rotl64(h0 ^ k, 23) * PW_P2 + PW_P3;
    h1 = pw_rotl64(h1 ^ k, 23) * PW_P2 + PW_P3;
    rem -= 4;
  }
  if (rem > 0) {
    uint32_t t = pw_tok_next32(&r);
    for (; rem > 0; --rem, t >>= 8) {
      const uint64_t k = (uint64_t)(t & 0xFFu) * PW_P5;
      h0 = pw_rotl64(h0 ^ k, 11) * PW_P1;
      h1 = pw_rotl64(h1 ^ k, 11) * PW_P1;
    }
  }
  PwHash128 out;
  out.lo = pw_avalanche(h0);
  out.hi = pw_avalanche(h1);
  return out;
}
