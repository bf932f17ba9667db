// encode_long.h — a long escaped value encoded by many workgroups: the chunked
// path of the resident writer (encode.hip) and the batch writer
// (encode_batch.hip). The window writer (encode_window.hip) carries the text it
// was measured with.
//
// A value of at least `long_value` bytes that needs escaping is cut into chunks
// of kLongChunk bytes, counted from the value's first 16-byte block, one
// workgroup per chunk:
//   1. the writer's values kernel stores the record's chunk count (0 for every
//      other record; 32 bits); an exclusive scan of the counts gives the chunk
//      ranges;
//   2. long_chunk_kernel<false>: every byte's output width by the local rule of
//      escape_width.h, summed per chunk;
//   3. long_fix_kernel: the wave that holds a long record scans its chunks'
//      sums, 64 at a time: a chunk's offset inside its value, and the value's
//      encoded length, added to the line's. Only the chunks that exist are
//      touched: an encode without a long value pays the scan of step 1 and
//      nothing that grows with the chunk tables;
//   4. the line writer writes the line's head and tail, leaves the value's
//      place in val_pos[record] and sets kLongPlaced in the record's chunk
//      count. A line that does not fit below out_cap is skipped and gets no
//      bit. A long value that keeps its length (valid UTF-8 and nothing else
//      to escape) is copied like a plain line by the wave writers, which tell
//      an escaped line by its length, and gets no bit there; the per-thread
//      writer of a file name past the LDS head looks at the count first, so
//      there such a value gets the bit and the chunk pass writes it: the same
//      bytes either way;
//   5. long_chunk_kernel<true>, for the records with the bit: per 4 KiB step a
//      workgroup scan of the lanes' width sums, then every lane writes its 16
//      bytes' expansions.
//
// POSITIONS. A writer's buffer need not be 16-byte aligned (the device forms
// take the caller's pointer), and nothing outside its n bytes may be read. So
// the kernels work in VIRTUAL positions: position v is the byte data[v - lo],
// where lo = the buffer's address modulo 16. A virtual position that is a
// multiple of 16 is then a 16-byte-aligned ADDRESS, and the readable positions
// are [lo, lo + n). A block or neighbouring dword that does not lie wholly
// inside them is assembled from byte loads clipped to them (long_load).
#pragma once
#include <stdint.h>

#include "encode_common.h"
#include "encode_window.h"  // kLongChunk, kLongStep, kLongValueDefault
#include "escape_width.h"

namespace dgrep {

// set in a record's chunk count once its line writer has left the value's
// place in val_pos: the chunk pass writes that value (a count stays below 2^31)
constexpr uint32_t kLongPlaced = 0x80000000u;

// the readable bytes of a writer's buffer, in virtual positions
struct LongSpan {
  const uint8_t* data;  // the byte at position lo
  uint64_t lo, hi;      // [lo, hi) = the buffer; lo = data's address & 15
};

DGREP_HD inline LongSpan long_span(const uint8_t* data, uint64_t n) {
  const uint64_t lo = uint64_t(reinterpret_cast<uintptr_t>(data) & 15u);
  return LongSpan{data, lo, lo + n};
}

// The ND dwords (1 or 4) at position pos, a multiple of 4 * ND, to q: one
// aligned load when they lie inside the buffer, else its bytes one by one and 0
// for every position outside it. No byte outside [lo, hi) is read.
template <int ND>
DGREP_HD inline void long_load(const LongSpan& s, uint64_t pos, uint32_t* q) {
  if (pos >= s.lo && pos + 4u * ND <= s.hi) {
    __builtin_memcpy(q, __builtin_assume_aligned(s.data + (pos - s.lo), 4 * ND), 4 * ND);
    return;
  }
  for (int k = 0; k < ND; ++k) q[k] = 0;
  for (uint32_t b = 0; b < 4u * ND; ++b) {
    const uint64_t p = pos + b;
    if (p >= s.lo && p < s.hi) q[b >> 2] |= uint32_t(s.data[p - s.lo]) << (8 * (b & 3));
  }
}

// the chunks of the value at positions [st, e)
DGREP_HD inline uint64_t long_chunk_count(uint64_t st, uint64_t e) {
  return (e - (st & ~uint64_t(15)) + kLongChunk - 1) / kLongChunk;
}

// Every long value has at least long_value bytes and at most len / kLongChunk +
// 2 chunks (its first and last blocks may be partial), and the values of a
// scan's records lie apart in the n bytes: the chunks number at most this.
// Records made by hand may overlap (the device forms do not check them): a
// value whose chunks do not fit the tables takes the one-lane path
// (long_fix_kernel), so the output is the same whatever the records.
inline uint64_t long_max_chunks(uint64_t n, uint64_t records, uint32_t long_value) {
  const uint64_t lv = long_value ? long_value : 1;
  return n / kLongChunk + 2 * (records < n / lv ? records : n / lv) + 2;
}

#if defined(__HIP_DEVICE_COMPILE__)
__device__ __forceinline__ uint32_t long_special4(const uint32_t* q) {
  return special_bytes(q[0]) | special_bytes(q[1]) | special_bytes(q[2]) | special_bytes(q[3]);
}
#else
inline uint32_t long_special4(const uint32_t* q) {  // the host's restatement of special_bytes over 16 bytes
  for (int k = 0; k < 16; ++k) {
    const uint32_t b = (q[k >> 2] >> (8 * (k & 3))) & 0xffu;
    if (b < 0x20 || b >= 0x80 || b == '"' || b == '\\' || b == '<' || b == '>' || b == '&') return 1;
  }
  return 0;
}
#endif

// One lane's 16-byte block at position blk of the value at [st, e): by32[1..4]
// = the block, by32[0] and by32[5] = the dwords before and after it where they
// belong to the value's blocks (A = st rounded down, E16 = e rounded up to 16).
// Returns the sum of the widths of the block's bytes that lie inside the value
// and their widths, 4 bits each; `plain`: all 16 inside the value, each 1 wide.
DGREP_HD inline uint32_t long_block_widths(const LongSpan& s, uint64_t st, uint64_t e, uint64_t blk, uint32_t (&by32)[6],
                                           uint64_t* widths, bool* plain) {
  const uint64_t A = st & ~uint64_t(15), E16 = (e + 15) & ~uint64_t(15);
  by32[0] = by32[5] = 0;
  *widths = 0;
  *plain = false;
  long_load<4>(s, blk, by32 + 1);
  if (blk >= st && blk + 16 <= e && long_special4(by32 + 1) == 0u) {
    *plain = true;  // ASCII with nothing to escape: every width is 1, whatever the neighbours
    return 16;
  }
  if (blk > A) long_load<1>(s, blk - 4, by32);
  if (blk + 16 < E16) long_load<1>(s, blk + 16, by32 + 5);
  uint8_t by[24];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int k = 0; k < 24; ++k) by[k] = uint8_t(by32[k >> 2] >> (8 * (k & 3)));
  uint32_t sum = 0;
  uint64_t w = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int k = 0; k < 16; ++k) {
    const uint64_t p = blk + uint64_t(k);
    if (p < st || p >= e) continue;
    const uint32_t before = uint32_t(p - st < 3 ? p - st : 3), after = uint32_t(e - 1 - p < 3 ? e - 1 - p : 3);
    const uint32_t wd = escape_width(by + k + 1, before, after);
    sum += wd;
    w |= uint64_t(wd) << (4 * k);
  }
  *widths = w;
  return sum;
}

// The block's expansions to o (what long_block_widths returned for it);
// returns the bytes written.
DGREP_HD inline uint32_t long_block_put(const uint32_t (&by32)[6], uint64_t e, uint64_t blk, uint64_t widths, bool plain,
                                        uint8_t* o) {
  if (plain) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int k = 0; k < 16; ++k) o[k] = uint8_t(by32[1 + (k >> 2)] >> (8 * (k & 3)));
    return 16;
  }
  uint8_t by[24];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int k = 0; k < 24; ++k) by[k] = uint8_t(by32[k >> 2] >> (8 * (k & 3)));
  uint8_t* const o0 = o;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int k = 0; k < 16; ++k) {
    const uint32_t wd = uint32_t(widths >> (4 * k)) & 15u;
    if (wd == 0) continue;  // outside the value, or swallowed
    const uint64_t p = blk + uint64_t(k);
    escape_put(by + k + 1, uint32_t(e - 1 - p < 3 ? e - 1 - p : 3), wd, o);
    o += wd;
  }
  return uint32_t(o - o0);
}

}  // namespace dgrep

#if defined(__HIPCC__)
#include <hipcub/hipcub.hpp>

#include <algorithm>

namespace dgrep {
namespace {

constexpr int kLongThreads = int(kLongStep / 16);  // a lane takes one 16-byte block per step
constexpr int kLongWaves = kLongThreads / 64;

// inclusive scan over the wave
__device__ __forceinline__ uint32_t wave_inclusive(uint32_t v, uint32_t lane) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t u = uint32_t(__shfl_up(int(v), d, 64));
    if (lane >= uint32_t(d)) v += u;
  }
  return v;
}

// One workgroup per chunk of a long value (grid-stride over the chunks).
// WRITE = false: chunk_sum[c] = the chunk's bytes' widths, summed.
// WRITE = true: the expansions to out, from val_pos[record] + the chunk's
// offset inside its value (chunk_pos, from long_fix_kernel).
// loc(i) = the position of record i's value. A chunk is written only if its
// record has kLongPlaced, which a line gets only when it fits below out_cap: no
// byte at or past out_cap is written.
template <bool WRITE, class Loc>
__global__ __launch_bounds__(kLongThreads) void long_chunk_kernel(LongSpan sp, Loc loc, const uint64_t* __restrict__ len,
                                                                  uint64_t count, const uint32_t* __restrict__ nchunks,
                                                                  const uint64_t* __restrict__ chunk_base,
                                                                  uint64_t max_chunks, uint32_t* chunk_sum,
                                                                  const uint64_t* __restrict__ chunk_pos,
                                                                  const uint64_t* __restrict__ val_pos, uint8_t* out) {
  __shared__ uint32_t wsum[kLongWaves];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
  const uint64_t total = min(chunk_base[count], max_chunks);
  for (uint64_t c = blockIdx.x; c < total; c += gridDim.x) {
    uint64_t lo = 0, hi = count;  // the last record whose first chunk is <= c: records without chunks share a base
    while (hi - lo > 1) {
      const uint64_t mid = (lo + hi) >> 1;
      if (chunk_base[mid] <= c) lo = mid; else hi = mid;
    }
    const uint64_t i = lo, st = loc(i), e = st + len[i];
    if (chunk_base[i + 1] > max_chunks) continue;  // the tables are full: one lane writes this value
    const uint64_t A = st & ~uint64_t(15), E16 = (e + 15) & ~uint64_t(15);
    const uint64_t cb = A + (c - chunk_base[i]) * kLongChunk, ce = min(cb + kLongChunk, E16);
    uint64_t obase = 0;
    if (WRITE) {
      if ((nchunks[i] & kLongPlaced) == 0u) continue;  // skipped or copied by the line writer (workgroup-uniform)
      obase = val_pos[i] + chunk_pos[c];
    }
    uint32_t mine = 0;  // WRITE = false: this lane's widths over all steps
    for (uint64_t it = cb; it < ce; it += kLongStep) {
      const uint64_t blk = it + 16u * tid;
      uint32_t by32[6];
      uint32_t sum = 0;
      uint64_t widths = 0;  // 4 bits per byte
      bool plain = false;
      if (blk < ce) sum = long_block_widths(sp, st, e, blk, by32, &widths, &plain);
      if (!WRITE) {
        mine += sum;
        continue;
      }
      // the step's exclusive scan over the workgroup
      const uint32_t inc = wave_inclusive(sum, lane);
      if (lane == 63) wsum[wv] = inc;
      __syncthreads();
      uint32_t before_me = inc - sum, step_total = 0;
#pragma unroll
      for (uint32_t k = 0; k < uint32_t(kLongWaves); ++k) {
        if (k < wv) before_me += wsum[k];
        step_total += wsum[k];
      }
      __syncthreads();  // wsum is rewritten next step
      if (blk < ce) long_block_put(by32, e, blk, widths, plain, out + obase + before_me);
      obase += step_total;
    }
    if (!WRITE) {
      const uint32_t inc = wave_inclusive(mine, lane);
      if (lane == 63) wsum[wv] = inc;
      __syncthreads();
      if (tid == 0) {
        uint32_t t = 0;  // at most 6 x kLongChunk
        for (uint32_t k = 0; k < uint32_t(kLongWaves); ++k) t += wsum[k];
        chunk_sum[c] = t;
      }
      __syncthreads();
    }
  }
}

// One thread per record, then the wave together for each of its long records:
// the chunks' sums, 64 at a time, become the chunks' offsets inside the value
// (chunk_pos), and their total the value's encoded length, which goes into its
// line's length. A value whose chunks did not fit the tables is measured here
// by its lane (json_body) and is no long value from here on. stats[0] += the
// long values, stats[1] += their chunks (both zeroed beforehand).
template <class Loc>
__global__ __launch_bounds__(kLongThreads) void long_fix_kernel(LongSpan sp, Loc loc, const uint64_t* len,
                                                                uint64_t count, uint32_t* nchunks,
                                                                const uint64_t* chunk_base, const uint32_t* chunk_sum,
                                                                uint64_t* chunk_pos, uint64_t max_chunks,
                                                                uint64_t* enc_len, uint64_t* stats) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t stride = uint64_t(gridDim.x) * kLongThreads;
  for (uint64_t i0 = uint64_t(blockIdx.x) * kLongThreads; i0 < count; i0 += stride) {  // workgroup-uniform trips
    const uint64_t i = i0 + threadIdx.x;
    uint32_t nc = i < count ? nchunks[i] : 0u;
    uint64_t c0 = 0;
    if (nc != 0u) {
      c0 = chunk_base[i];
      if (c0 + nc > max_chunks) {
        enc_len[i] += json_body<false>(sp.data + (loc(i) - sp.lo), len[i], nullptr) - len[i];
        nchunks[i] = nc = 0;
      }
    }
    const uint64_t m = __ballot(nc != 0u);
    if (m == 0ull) continue;  // wave-uniform: the usual case, no long value among the wave's 64 records
    for (uint64_t left = m; left != 0ull; left &= left - 1) {
      const int r = __ffsll((long long)left) - 1;
      const uint32_t cnt = uint32_t(__shfl(int(nc), r, 64));
      const uint64_t first = __shfl(c0, r, 64);
      uint64_t running = 0;
      for (uint32_t k0 = 0; k0 < cnt; k0 += 64u) {  // wave-uniform trips
        const uint32_t k = k0 + lane;
        const uint32_t v = k < cnt ? chunk_sum[first + k] : 0u;
        const uint32_t inc = wave_inclusive(v, lane);  // 64 chunks' sums: below 2^32
        if (k < cnt) chunk_pos[first + k] = running + (inc - v);
        running += uint32_t(__shfl(int(inc), 63, 64));
      }
      if (int(lane) == r) enc_len[i] += running - len[i];
    }
    uint32_t sum = nc;  // (max_chunks is far below 2^32 / 64)
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) sum += uint32_t(__shfl_xor(int(sum), d, 64));
    if (lane == uint32_t(__ffsll((long long)m) - 1)) {
      atomicAdd(reinterpret_cast<unsigned long long*>(stats), (unsigned long long)__popcll(m));
      atomicAdd(reinterpret_cast<unsigned long long*>(stats + 1), (unsigned long long)sum);
    }
  }
}

struct LongWiden {
  __host__ __device__ uint64_t operator()(uint32_t x) const { return x; }
};
using LongCounts = hipcub::TransformInputIterator<uint64_t, LongWiden, const uint32_t*>;

inline size_t long_align256(size_t x) { return (x + 255) & ~size_t(255); }

// The chunk tables, carved from a writer's scratch: per record its chunk count
// and first chunk (count + 1 entries: the last is the total), per chunk its
// width sum and its offset inside its value.
struct LongTables {
  uint32_t *nchunks, *chunk_sum;
  uint64_t *chunk_base, *chunk_pos;  // (64 bits: the counts of records made by hand may add up past 2^32)
  uint64_t max_chunks;
  static size_t bytes(uint64_t n, uint64_t max_chunks) {
    return long_align256((n + 1) * 4) + long_align256((n + 1) * 8) + long_align256((max_chunks + 1) * 4) +
           long_align256((max_chunks + 1) * 8);
  }
  template <class Carver>
  LongTables(Carver& c, uint64_t n, uint64_t max_chunks_)
      : nchunks(c.template take<uint32_t>(n + 1)), chunk_base(c.template take<uint64_t>(n + 1)),
        chunk_sum(c.template take<uint32_t>(max_chunks_ + 1)), chunk_pos(c.template take<uint64_t>(max_chunks_ + 1)),
        max_chunks(max_chunks_) {}
};

// hipcub's temporary bytes for long_measure's scan (size-only call)
inline hipError_t long_scan_tmp(uint64_t n, size_t* tmp, hipStream_t s) {
  return hipcub::DeviceScan::ExclusiveSum(nullptr, *tmp, LongCounts(nullptr, LongWiden()), (uint64_t*)nullptr, n + 1, s);
}

inline int long_grid_for(uint64_t max_chunks) { return int(max_chunks < 4096 ? max_chunks : 4096); }

// Steps 1 to 3 over n >= 1 records whose chunk counts stand in q.nchunks[0, n]
// (the last entry 0): the long values' encoded lengths go into enc_len, their
// number and their chunks' to stats[0..1] (both zeroed beforehand).
template <class Loc>
hipError_t long_measure(const LongSpan& sp, Loc loc, const uint64_t* len, uint64_t n, const LongTables& q,
                        uint64_t* enc_len, uint64_t* stats, void* t, size_t tmp, hipStream_t s) {
  hipError_t e;
  size_t tb = tmp;
  if ((e = hipcub::DeviceScan::ExclusiveSum(t, tb, LongCounts(q.nchunks, LongWiden()), q.chunk_base, n + 1, s)) !=
      hipSuccess)
    return e;
  hipLaunchKernelGGL((long_chunk_kernel<false, Loc>), dim3(long_grid_for(q.max_chunks)), dim3(kLongThreads), 0, s, sp,
                     loc, len, n, q.nchunks, q.chunk_base, q.max_chunks, q.chunk_sum, nullptr, nullptr, nullptr);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  const int grid = int(std::min<uint64_t>((n + kLongThreads - 1) / kLongThreads, 8192));
  hipLaunchKernelGGL((long_fix_kernel<Loc>), dim3(grid), dim3(kLongThreads), 0, s, sp, loc, len, n, q.nchunks,
                     q.chunk_base, q.chunk_sum, q.chunk_pos, q.max_chunks, enc_len, stats);
  return hipGetLastError();
}

// Step 5, after the line writer has left every long value's place in val_pos.
template <class Loc>
hipError_t long_write(const LongSpan& sp, Loc loc, const uint64_t* len, uint64_t n, const LongTables& q,
                      const uint64_t* val_pos, uint8_t* out, hipStream_t s) {
  hipLaunchKernelGGL((long_chunk_kernel<true, Loc>), dim3(long_grid_for(q.max_chunks)), dim3(kLongThreads), 0, s, sp,
                     loc, len, n, q.nchunks, q.chunk_base, q.max_chunks, nullptr, q.chunk_pos, val_pos, out);
  return hipGetLastError();
}

}  // namespace
}  // namespace dgrep
#endif  // __HIPCC__
