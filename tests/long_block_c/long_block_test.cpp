// The chunked long-value path's host side (csrc/kernels/encode_long.h) under
// ASan + UBSan: the clipped block assembly (long_load, long_block_widths,
// long_block_put) and a restatement of the two chunk passes -- chunk count,
// width sums per chunk, their exclusive scan, the write at the offsets -- over
// buffers of exactly n bytes at every address phase, compared byte for byte
// with json_body<true> (encode_common.h). A read before the buffer's first or
// past its last byte is an ASan report: the bytes before it are poisoned, the
// bytes behind it are malloc's red zone.
//
// Inputs: a value of 1..48 bytes over the edge alphabet at each of the 16
// address phases of its start, with each of the 16 phases of the buffer's end,
// at the buffer's first byte and 5 bytes in; values of 16 KiB +- 17 bytes at
// start phases 0, 1 and 15; 2,000 seeded random values. Prints "OK <count>
// inputs".
#include <sanitizer/asan_interface.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "encode_long.h"

using namespace dgrep;

// window_part_cases.EDGE_BYTES
static const uint8_t kEdge[] = {0x00, 0x22, 0x41, 0x7F, 0x80, 0x8F, 0x90, 0x9F, 0xA0, 0xA8, 0xA9, 0xBF,
                                0xC0, 0xC2, 0xDF, 0xE0, 0xE2, 0xED, 0xEF, 0xF0, 0xF4, 0xF5, 0xFF};
static const size_t kEdgeN = sizeof kEdge;

static uint64_t g_inputs = 0;

// The buffer is pre + len + post bytes whose first byte lies at address phase
// `phase`; the value is its bytes [pre, pre + len). `fill` gives every byte.
static void run(uint32_t phase, size_t pre, size_t len, size_t post, std::mt19937& rng, bool edge_only) {
  const size_t n = pre + len + post;
  uint8_t* raw = static_cast<uint8_t*>(malloc(phase + n));  // malloc's 16-byte alignment: raw + phase has that phase
  if (!raw || (reinterpret_cast<uintptr_t>(raw) & 15u) != 0) { fprintf(stderr, "unaligned malloc\n"); exit(2); }
  uint8_t* data = raw + phase;
  for (size_t k = 0; k < n; ++k) {
    uint8_t b = (edge_only || (rng() & 1u)) ? kEdge[rng() % kEdgeN] : uint8_t(rng());
    data[k] = b == '\n' ? 'n' : b;
  }
  ASAN_POISON_MEMORY_REGION(raw, phase);

  const LongSpan sp = long_span(data, n);
  if (sp.lo != phase || sp.hi != phase + n) { fprintf(stderr, "long_span\n"); exit(2); }
  const uint64_t st = sp.lo + pre, e = st + len;
  const uint64_t A = st & ~uint64_t(15), E16 = (e + 15) & ~uint64_t(15);
  const uint64_t nch = long_chunk_count(st, e);
  if (nch != (E16 - A + kLongChunk - 1) / kLongChunk || nch > len / kLongChunk + 2) {
    fprintf(stderr, "chunk count %llu of a value of %zu bytes\n", (unsigned long long)nch, len);
    exit(1);
  }
  // pass 1: the chunks' width sums
  std::vector<uint64_t> sum(nch + 1, 0), pos(nch + 1, 0);
  for (uint64_t c = 0; c < nch; ++c) {
    const uint64_t cb = A + c * kLongChunk, ce = cb + kLongChunk < E16 ? cb + kLongChunk : E16;
    for (uint64_t blk = cb; blk < ce; blk += 16) {
      uint32_t by32[6];
      uint64_t widths;
      bool plain;
      sum[c] += long_block_widths(sp, st, e, blk, by32, &widths, &plain);
    }
  }
  for (uint64_t c = 0; c < nch; ++c) pos[c + 1] = pos[c] + sum[c];
  const uint64_t total = pos[nch];
  // the reference
  const uint64_t want_n = json_body<false>(data + pre, len, nullptr);
  std::vector<uint8_t> want(want_n + 1), got(total + 1, 0xA5);
  json_body<true>(data + pre, len, want.data());
  // pass 2: every chunk writes at its offset, in reverse order (no chunk leans on another's pointer)
  for (uint64_t c = nch; c-- > 0;) {
    const uint64_t cb = A + c * kLongChunk, ce = cb + kLongChunk < E16 ? cb + kLongChunk : E16;
    uint8_t* o = got.data() + pos[c];
    for (uint64_t blk = cb; blk < ce; blk += 16) {
      uint32_t by32[6];
      uint64_t widths;
      bool plain;
      const uint32_t w = long_block_widths(sp, st, e, blk, by32, &widths, &plain);
      const uint32_t put = long_block_put(by32, e, blk, widths, plain, o);
      if (put != w) { fprintf(stderr, "a block of width %u wrote %u bytes\n", w, put); exit(1); }
      o += put;
    }
    if (uint64_t(o - got.data()) != pos[c + 1]) { fprintf(stderr, "chunk %llu ends elsewhere\n", (unsigned long long)c); exit(1); }
  }
  if (total != want_n || memcmp(got.data(), want.data(), total) != 0 || got[total] != 0xA5) {
    fprintf(stderr, "mismatch: phase %u pre %zu len %zu post %zu: %llu bytes, json_body %llu\n", phase, pre, len, post,
            (unsigned long long)total, (unsigned long long)want_n);
    exit(1);
  }
  ASAN_UNPOISON_MEMORY_REGION(raw, phase);
  free(raw);
  ++g_inputs;
}

int main() {
  std::mt19937 rng(2026);
  for (uint32_t ps = 0; ps < 16; ++ps)       // the address phase of the value's first byte
    for (size_t pre = 0; pre <= 5; pre += 5)  // at the buffer's first byte, and 5 bytes in
      for (size_t len = 1; len <= 48; ++len)
        for (size_t post = 0; post < 16; ++post)  // every phase of the buffer's end
          run((ps + 16 - uint32_t(pre)) & 15u, pre, len, post, rng, true);
  for (uint32_t ps : {0u, 1u, 15u})
    for (size_t len = kLongChunk - 17; len <= kLongChunk + 17; ++len) run(ps, 0, len, 0, rng, false);
  for (int k = 0; k < 2000; ++k) {
    const size_t len = 1 + rng() % (k % 50 == 0 ? 40000 : 3000);
    run(rng() & 15u, rng() % 20, len, rng() % 20, rng, false);
  }
  printf("OK %llu inputs\n", (unsigned long long)g_inputs);
  return 0;
}
