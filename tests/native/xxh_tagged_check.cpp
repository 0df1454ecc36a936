// Stand-alone check of pw_xxh64_tagged2 (xxhash_common.h) against
// pw_xxh64_bytes over the concatenated message tag || bytes, for both seeds.
// Built with -fsanitize=address,undefined by tests/test_xxh_tagged_host.py:
// every buffer is a heap block that ends exactly at the buffer's last byte
// (and, for an aligned base, begins exactly at its first), so a load outside
// [base, base + nbytes) lands in a redzone and aborts the run.
//
// A base that is not 4-byte aligned cannot begin a heap block: the m bytes in
// front of it belong to the same block, so the sanitizer does not see a read
// of them, and the hash does not show one either (the reader shifts those
// low bytes out).  For that start, check_boundary_dwords() calls pw_tok_dword
// itself on the dword that begins before the base and compares it with one
// put together from the in-range bytes only; the bytes in front are non-zero
// junk, so a whole-dword load there gives another value.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "xxhash_common.h"

static uint64_t rng_state = 0x243F6A8885A308D3ULL;
static uint8_t rnd8() {
  rng_state = rng_state * 6364136223846793005ULL + 1442695040888963407ULL;
  return (uint8_t)(rng_state >> 56);
}

static long checked = 0;

// token base[a : a+len] inside a buffer of nbytes at misalignment mis
static int check(int64_t nbytes, int64_t a, int64_t len, int mis, uint64_t tag) {
  uint8_t* block = (uint8_t*)malloc((size_t)(nbytes + mis) ? (size_t)(nbytes + mis) : 1);
  uint8_t* base = block + mis;
  for (int j = 0; j < mis; ++j) block[j] = 0xA5 ^ (uint8_t)j;
  for (int64_t j = 0; j < nbytes; ++j) base[j] = rnd8();
  uint8_t* msg = (uint8_t*)malloc((size_t)(8 + len));
  memcpy(msg, &tag, 8);
  if (len) memcpy(msg + 8, base + a, (size_t)len);
  const uint64_t want_lo = pw_xxh64_bytes(msg, 8 + len, PW_SEED_LO);
  const uint64_t want_hi = pw_xxh64_bytes(msg, 8 + len, PW_SEED_HI);
  const PwHash128 got = pw_xxh64_tagged2(base, nbytes, a, len, tag);
  free(msg);
  free(block);
  ++checked;
  if (got.lo != want_lo || got.hi != want_hi) {
    fprintf(stderr,
            "MISMATCH nbytes=%lld a=%lld len=%lld mis=%d: got %016llx %016llx "
            "want %016llx %016llx\n",
            (long long)nbytes, (long long)a, (long long)len, mis,
            (unsigned long long)got.lo, (unsigned long long)got.hi,
            (unsigned long long)want_lo, (unsigned long long)want_hi);
    return 1;
  }
  return 0;
}

// pw_tok_dword on the dwords that straddle the buffer's first and last byte
static int check_boundary_dwords() {
  int bad = 0;
  for (int mis = 1; mis <= 3; ++mis)
    for (int64_t nbytes = 1; nbytes <= 8; ++nbytes) {
      uint8_t* block = (uint8_t*)malloc((size_t)(nbytes + mis));
      uint8_t* base = block + mis;
      for (int j = 0; j < mis; ++j) block[j] = 0xA5 ^ (uint8_t)j;
      for (int64_t j = 0; j < nbytes; ++j) base[j] = (uint8_t)(rnd8() | 1);
      const uintptr_t blo = (uintptr_t)base, bhi = blo + (uintptr_t)nbytes;
      const uintptr_t qs[2] = {(uintptr_t)block, (bhi - 1) & ~(uintptr_t)3};
      for (int w = 0; w < 2; ++w) {
        uint32_t want = 0;
        for (int j = 0; j < 4; ++j)
          if (qs[w] + j >= blo && qs[w] + j < bhi)
            want |= (uint32_t)(*(const uint8_t*)(qs[w] + j)) << (8 * j);
        const uint32_t got = pw_tok_dword(qs[w], bhi, blo, bhi);
        ++checked;
        if (got != want) {
          fprintf(stderr, "DWORD mis=%d nbytes=%lld which=%d: got %08x want %08x\n",
                  mis, (long long)nbytes, w, got, want);
          ++bad;
        }
      }
      free(block);
    }
  return bad;
}

int main() {
  int bad = check_boundary_dwords();
  const uint64_t tags[2] = {5ULL, 0xF00DFACE12345678ULL};
  for (int64_t len = 0; len <= 130; ++len)
    for (int64_t off = 0; off <= 7; ++off)
      for (int mis = 0; mis <= 3; ++mis) {
        const uint64_t tag = tags[(len + off + mis) & 1];
        // token at the buffer's very first byte, `off` bytes behind it
        bad += check(len + off, 0, len, mis, tag);
        // token that ends on the buffer's very last byte
        bad += check(len + off, off, len, mis, tag);
        // slack on both sides
        bad += check(len + off + 9, off, len, mis, tag);
      }
  if (bad) {
    fprintf(stderr, "%d mismatches\n", bad);
    return 1;
  }
  printf("ok %ld\n", checked);
  return 0;
}
