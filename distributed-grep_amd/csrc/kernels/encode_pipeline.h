// encode_pipeline.h — what the resident partition writer (encode.hip) and the
// batch writer (encode_batch.hip) share, once: the wave's value sweep, the key
// hash and plain length, the per-thread line writer, the plain line's dword
// assembly with the head byte fetched through a callable (write_plain_line),
// gather_len_kernel, the grids, the scratch carver, the per-record tables and
// the host's "sort by key, gather the lengths, scan them". A long escaped value
// takes the chunked path of encode_long.h in both. The window writer
// (encode_window.hip) still carries its own copy (DESIGN 3.13 says why). All
// of it sits in an unnamed namespace, as in reduce_common.h.
#pragma once
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>

#include "encode_common.h"
#include "encode_long.h"

namespace dgrep {
namespace {

constexpr int kEncThreads = 256;
constexpr int kEncWaves = kEncThreads / 64;
constexpr uint32_t kHeadMax = 2048;  // LDS bytes of a staged line head `{"Key":"<file> (line number #`

// One WAVE per value: its bytes data[st, e) are tested 4 per lane (aligned
// dwords, SWAR) and a ballot decides, so consecutive lanes read consecutive
// dwords and a value is one coalesced sweep. Returns whether anything needs
// escaping (wave-uniform). `early` (wave-uniform): leave at the first escape
// seen, so that a long escaped value is not swept to its end by this one wave.
__device__ __forceinline__ bool value_needs_escape(const uint8_t* data, uint64_t n, uint64_t st, uint64_t e,
                                                   uint32_t lane, bool early) {
  bool bad = false;
  for (uint64_t w = (st & ~uint64_t(3)) + 4u * lane; w < e; w += 256) {
    uint32_t x;
    if (w + 4 <= n) {
      x = *reinterpret_cast<const uint32_t*>(data + w);
    } else {  // the buffer's last partial dword: no read past n
      x = 0x20202020u;
      for (uint32_t k = 0; w + k < n; ++k) x = (x & ~(0xffu << (8 * k))) | (uint32_t(data[w + k]) << (8 * k));
    }
    const uint32_t in = (w >= st && w + 4 <= e) ? 0x80808080u : range_mask(w, st, e);
    bad = bad || (special_bytes(x) & in) != 0u;
    // (every lane still in the loop sees the same ballot and leaves with the others)
    if (early && __ballot(bad) != 0ull) break;
  }
  return __ballot(bad) != 0ull;
}

// What a values kernel does with record i once its wave knows whether the
// value data[st, e) needs escaping: a long escaped value (at least long_value
// bytes; vst = its position, encode_long.h) only gets its chunk count, a short
// one its exact encoded length from json_body (lane 0).
__device__ __forceinline__ void value_measured(const uint8_t* data, uint64_t st, uint64_t e, uint64_t vst, bool escaped,
                                               uint32_t long_value, uint32_t lane, uint64_t* enc_len,
                                               uint32_t* nchunks) {
  if (lane != 0) return;
  if (escaped && e - st >= long_value) {
    *nchunks = uint32_t(long_chunk_count(vst, vst + (e - st)));
  } else {
    *nchunks = 0;
    if (escaped) *enc_len += json_body<false>(data + st, e - st, nullptr) - (e - st);
  }
}

// ihash of the key "<file> (line number #<line_no>)": FNV-1a continued from h0
// (the state after "<file> (line number #") over the decimal digits and ')'.
// d[0, nd) = the digits (digits_of).
__device__ __forceinline__ uint32_t key_ihash(uint32_t h0, const uint8_t (&d)[20], uint32_t nd) {
  uint32_t h = h0;
  for (uint32_t k = 0; k < nd; ++k) h = fnv_step(h, uint32_t('0') + d[k]);
  h = fnv_step(h, uint32_t(')'));
  return h & 0x7fffffffu;
}

// the encoded line's length when the value (L bytes) has nothing to escape;
// F = the escaped file name's bytes, nd = the line number's digits
__device__ __forceinline__ uint64_t plain_line_len(uint32_t F, uint32_t nd, uint64_t L) {
  return kFixedBytes + F + nd + L;
}

// byte k of the line head `{"Key":"<name> (line number #` (k < 8 + F + 15)
template <class Index>
__device__ __forceinline__ uint8_t head_byte(const uint8_t* name, uint32_t F, Index k) {
  return k < 8u ? uint8_t("{\"Key\":\""[k]) : k < 8u + F ? name[k - 8u] : uint8_t(" (line number #"[k - 8u - F]);
}

// what a lane wrote to the wave's LDS rows becomes visible to its other lanes
__device__ __forceinline__ void wave_publish_lds() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// One thread writes one record's line of enc bytes at out + P (the values that need
// escaping, and every line of a file name past the LDS head). st and len are
// REFERENCES on purpose: a caller that passes a table entry (a.start[i]) has
// it loaded where the line needs it, after the head's stores, which loads
// cannot move past; loaded before the call they cost the resident write kernel
// 27 VGPRs. nchunks[i] = the record's chunk count (encode_long.h): not 0 for a
// long value, whose bytes are left to the chunk pass; its place in out goes to
// val_pos[i] and kLongPlaced into the count. The wave writers call it behind
// their loop over the wave's lines, every escaped line's lane at once: called
// inside that loop its registers were the loop's (123 VGPRs instead of 96 in
// the resident write kernel, one wave per SIMD fewer).
__device__ void write_line_thread(const uint8_t* name, uint32_t F, uint64_t line_no, const uint8_t* data,
                                  const uint64_t& st, const uint64_t& len, uint8_t* out, uint64_t P, uint64_t enc,
                                  uint32_t* nchunks, uint64_t* val_pos, uint64_t i) {
  uint8_t* o = out + P;
  put_str(o, "{\"Key\":\"");
  for (uint32_t k = 0; k < F; ++k) *o++ = name[k];
  put_str(o, " (line number #");
  uint8_t d[20];
  const uint32_t nd = digits_of(line_no, d);
  for (uint32_t k = 0; k < nd; ++k) *o++ = uint8_t('0' + d[k]);
  put_str(o, ")\",\"Value\":\"");
  const uint64_t L = len;
  if (nchunks[i] != 0u) {
    val_pos[i] = uint64_t(o - out);
    nchunks[i] |= kLongPlaced;
    o += enc - plain_line_len(F, nd, 0);
  } else if (enc == plain_line_len(F, nd, L)) {
    copy_bytes(o, data + st, L);
    o += L;
  } else {
    o += json_body<true>(data + st, L, o);
  }
  put_str(o, "\"}\n");
}

// One WAVE writes one plain line (nothing to escape): T bytes at out + P, the
// value being data[src, src + L). Lane l builds the line's output dwords
// (P >> 2) + l + 64k from its five pieces -- the head `{"Key":"<file> (line
// number #` (A bytes, byte o from head(o)), the nd digits (digit_row),
// `)","Value":"`, the value bytes, `"}\n`. A dword wholly inside the value is
// one unaligned read of the buffer: two aligned dwords + v_alignbyte, taken
// only when the second one ends before the buffer's n bytes do. The first and
// last dwords of a line, shared with its neighbours, are stored byte by byte.
template <class Head>
__device__ __forceinline__ void write_plain_line(const uint8_t* data, uint64_t n, uint8_t* out, uint64_t P, uint64_t T,
                                                 uint64_t src, uint64_t L, uint32_t A, uint32_t nd,
                                                 const uint8_t* digit_row, uint32_t lane, Head head) {
  const uint64_t V0 = uint64_t(A) + nd + 12u;  // line offset of the first value byte
  const uint64_t d0 = P >> 2, d1 = (P + T + 3) >> 2;
  for (uint64_t d = d0 + lane; d < d1; d += 64) {
    const uint64_t q0 = 4u * d;
    const int64_t o0 = int64_t(q0) - int64_t(P);           // line offset of the dword's byte 0
    const uint64_t s0 = src + uint64_t(o0 - int64_t(V0));  // buffer position of byte 0 if it were value
    if (o0 >= int64_t(V0) && uint64_t(o0) + 4u <= V0 + L && ((s0 + 3) | 3u) < n) {
      const uint32_t sh = uint32_t(s0 & 3u);
      const uint32_t* w = reinterpret_cast<const uint32_t*>(data + (s0 & ~uint64_t(3)));
      const uint32_t lo = w[0], hi = sh ? w[1] : 0u;
      *reinterpret_cast<uint32_t*>(out + q0) = __builtin_amdgcn_alignbyte(hi, lo, sh);
      continue;
    }
    uint32_t word = 0, have = 0;
#pragma unroll
    for (uint32_t b = 0; b < 4; ++b) {
      const int64_t ob = o0 + int64_t(b);
      if (ob < 0 || uint64_t(ob) >= T) continue;
      const uint64_t o = uint64_t(ob);
      uint32_t ch;
      if (o < A) ch = head(o);
      else if (o < uint64_t(A) + nd) ch = uint32_t('0') + digit_row[o - A];
      else if (o < V0) ch = uint8_t(")\",\"Value\":\""[o - A - nd]);
      else if (o < V0 + L) ch = data[src + (o - V0)];
      else ch = uint8_t("\"}\n"[o - V0 - L]);
      word |= ch << (8 * b);
      have |= 1u << b;
    }
    if (have == 15u) {
      *reinterpret_cast<uint32_t*>(out + q0) = word;
    } else {
      for (uint32_t b = 0; b < 4; ++b)
        if (have & (1u << b)) out[q0 + b] = uint8_t(word >> (8 * b));
    }
  }
}

__global__ __launch_bounds__(kEncThreads) void gather_len_kernel(const uint32_t* idx, const uint64_t* enc_len,
                                                                 uint64_t* len_sorted, uint64_t count) {
  for (uint64_t j = uint64_t(blockIdx.x) * kEncThreads + threadIdx.x; j < count; j += uint64_t(gridDim.x) * kEncThreads)
    len_sorted[j] = enc_len[idx[j]];
}

inline size_t align256(size_t x) { return (x + 255) & ~size_t(255); }
inline int grid_for(uint64_t n) { return int(std::min<uint64_t>((n + kEncThreads - 1) / kEncThreads, 8192)); }
// one wave per record: 4 records per workgroup, at most 8 resident-sized rounds of the chip
inline int wave_grid_for(uint64_t n) { return int(std::min<uint64_t>((n + 3) / 4, 16384)); }
// one wave per 64 records
inline int wave64_grid_for(uint64_t n) { return int(std::min<uint64_t>((n + 255) / 256, 4096)); }

// the smallest end_bit with keys < 2^end_bit, at least 1
inline int key_bits(uint64_t keys) {
  int end_bit = 1;
  while ((1ull << end_bit) < keys) ++end_bit;
  return end_bit;
}

// hands out a caller's scratch in 256-byte-aligned pieces
struct ScratchCarver {
  uint8_t* p;
  template <class T>
  T* take(size_t count) {
    T* q = reinterpret_cast<T*>(p);
    p += align256(count * sizeof(T));
    return q;
  }
};

// The per-record tables of every writer, carved in this order: the sort key
// (partition or cell) and the record index before and after the sort, the
// encoded lengths in record and in sorted order, the lines' byte offsets.
template <class Key>
struct LineTables {
  Key *key_in, *key_out;
  uint32_t *idx_in, *idx_out;
  uint64_t *enc_len, *len_sorted, *pos;
  static size_t bytes(uint64_t n) {
    return 2 * align256(n * sizeof(Key)) + 2 * align256(n * 4) + 3 * align256(n * 8);
  }
  LineTables(ScratchCarver& c, uint64_t n)
      : key_in(c.take<Key>(n)), key_out(c.take<Key>(n)), idx_in(c.take<uint32_t>(n)), idx_out(c.take<uint32_t>(n)),
        enc_len(c.take<uint64_t>(n)), len_sorted(c.take<uint64_t>(n)), pos(c.take<uint64_t>(n)) {}
};

// hipcub's temporary bytes for sort_gather_scan over n records (size-only calls)
template <class Key>
hipError_t sort_gather_scan_tmp(uint64_t n, int end_bit, size_t* tmp, hipStream_t s) {
  size_t sort_tmp = 0, scan_tmp = 0;
  hipError_t e = hipcub::DeviceRadixSort::SortPairs(nullptr, sort_tmp, (Key*)nullptr, (Key*)nullptr, (uint32_t*)nullptr,
                                                    (uint32_t*)nullptr, n, 0, end_bit, s);
  if (e != hipSuccess) return e;
  e = hipcub::DeviceScan::ExclusiveSum(nullptr, scan_tmp, (uint64_t*)nullptr, (uint64_t*)nullptr, n, s);
  *tmp = std::max(sort_tmp, scan_tmp);
  return e;
}

// The pipeline's middle: a stable radix sort of (key, record) over end_bit bits
// keeps line order inside a key; the lengths gathered in sorted order and
// scanned give every line's byte offset. t: tmp bytes of temporary storage.
template <class Key>
hipError_t sort_gather_scan(const LineTables<Key>& q, uint64_t n, int end_bit, void* t, size_t tmp, hipStream_t s) {
  hipError_t e;
  size_t tb = tmp;
  if ((e = hipcub::DeviceRadixSort::SortPairs(t, tb, q.key_in, q.key_out, q.idx_in, q.idx_out, n, 0, end_bit, s)) !=
      hipSuccess)
    return e;
  hipLaunchKernelGGL(gather_len_kernel, dim3(grid_for(n)), dim3(kEncThreads), 0, s, q.idx_out, q.enc_len, q.len_sorted,
                     n);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  tb = tmp;
  return hipcub::DeviceScan::ExclusiveSum(t, tb, q.len_sorted, q.pos, n, s);
}

}  // namespace
}  // namespace dgrep
