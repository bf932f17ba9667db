// encode_window.hip — one window's Map output as partition-major
// json.Encoder lines: the writer of a streamed map task.
//
// The pipeline is encode.hip's (measure, stable radix sort by partition, scan,
// bounds, write), over the records of ONE window of a dgrep_stream, with two
// differences.
//
// (a) Coordinates. The records are the window's own (line_no and start as the
// window's scan returned them, so start indexes the window buffer); the
// stream's line_base is added wherever the line number is hashed or printed.
//
// (b) Long escaped values. encode.hip measures a value that needs escaping with
// one lane (json_body<false>) and writes it with one lane (json_body<true>):
// fine for a log line, a cliff for a 64 MiB line of minified JSON. Here a value
// of at least `long_value` bytes that needs escaping is cut into chunks of
// kLongChunk bytes (aligned to 16 from the value's first 16-byte block), one
// workgroup per chunk:
//   1. long_chunk_kernel<false>: every byte's output width by the local rule of
//      escape_width.h, summed per chunk;
//   2. an exclusive scan of the chunk sums (hipcub): a chunk's offset inside its
//      value, and the value's encoded length for the line scan;
//   3. long_chunk_kernel<true>: per 4 KiB step a workgroup scan of the lanes'
//      width sums, then every lane writes its 16 bytes' expansions.
// The value is read twice and the output written once. Which record a chunk
// belongs to comes from an exclusive scan of the per-record chunk counts
// (binary search): no atomics, no list built by appending. The line's head and
// tail are still written by the line writer, which leaves the value's place in
// the output to the chunk pass. Short values and long plain values are written
// exactly as encode_write_kernel writes them.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include "encode_common.h"
#include "encode_window.h"
#include "escape_width.h"

namespace dgrep {

namespace {
constexpr int kEncThreads = 256;
constexpr uint64_t kNoPos = ~uint64_t(0);

__global__ __launch_bounds__(kEncThreads) void win_measure_kernel(WindowEncodeArgs wa, uint16_t* part, uint32_t* idx,
                                                                  uint64_t* enc_len, uint64_t* nchunks) {
  const EncodeArgs& a = wa.e;
  if (blockIdx.x == 0 && threadIdx.x == 0) nchunks[a.count] = 0;  // the scan's last entry: the total
  for (uint64_t i = uint64_t(blockIdx.x) * kEncThreads + threadIdx.x; i < a.count;
       i += uint64_t(gridDim.x) * kEncThreads) {
    uint8_t d[20];
    const uint32_t nd = digits_of(wa.line_base + a.line_no[i], d);
    uint32_t h = a.key_hash0;
    for (uint32_t k = 0; k < nd; ++k) h = fnv_step(h, uint32_t('0') + d[k]);
    h = fnv_step(h, uint32_t(')'));
    part[i] = uint16_t((h & 0x7fffffffu) % a.nreduce);
    idx[i] = uint32_t(i);
    enc_len[i] = kFixedBytes + a.fname_json_len + nd + a.len[i];
  }
}

// One WAVE per record, as encode_values_kernel: SWAR test of the value's bytes,
// a ballot decides. A value with anything to escape is measured by lane 0 if it
// is short; a long one only gets its chunk count (nchunks[i] != 0 marks it).
__global__ __launch_bounds__(kEncThreads) void win_values_kernel(WindowEncodeArgs wa, uint64_t* enc_len,
                                                                 uint64_t* nchunks) {
  const EncodeArgs& a = wa.e;
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t waves = uint64_t(gridDim.x) * (kEncThreads / 64);
  for (uint64_t i = uint64_t(blockIdx.x) * (kEncThreads / 64) + (threadIdx.x >> 6); i < a.count; i += waves) {
    const uint64_t st = a.start[i], e = st + a.len[i];
    bool bad = false;
    for (uint64_t w = (st & ~uint64_t(3)) + 4u * lane; w < e; w += 256) {
      uint32_t x;
      if (w + 4 <= a.n) {
        x = *reinterpret_cast<const uint32_t*>(a.data + w);
      } else {  // the region's last partial dword: no read past n
        x = 0x20202020u;
        for (uint32_t k = 0; w + k < a.n; ++k) x = (x & ~(0xffu << (8 * k))) | (uint32_t(a.data[w + k]) << (8 * k));
      }
      const uint32_t in = (w >= st && w + 4 <= e) ? 0x80808080u : range_mask(w, st, e);
      bad = bad || (special_bytes(x) & in) != 0u;
      // one escape decides: a long escaped value is not swept to its end by this one wave
      // (every lane still in the loop sees the same ballot and leaves with the others)
      if (__ballot(bad) != 0ull) break;
    }
    const bool escaped = __ballot(bad) != 0ull;  // wave-uniform
    if (lane != 0) continue;
    if (escaped && e - st >= wa.long_value) {
      nchunks[i] = (e - (st & ~uint64_t(15)) + kLongChunk - 1) / kLongChunk;
    } else {
      nchunks[i] = 0;
      if (escaped) enc_len[i] += json_body<false>(a.data + st, e - st, nullptr) - (e - st);
    }
  }
}

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
// offset inside its value (chunk_pos = the exclusive scan of chunk_sum).
// A lane takes one aligned 16-byte block per step; its bytes' windows reach 3
// bytes into the dwords before and after, which are read only where they lie
// inside [value's first block, the value's end rounded up to 16).
template <bool WRITE>
__global__ __launch_bounds__(kEncThreads) void long_chunk_kernel(const uint8_t* __restrict__ data,
                                                                 const uint64_t* __restrict__ start,
                                                                 const uint64_t* __restrict__ len, uint64_t count,
                                                                 const uint64_t* __restrict__ chunk_base,
                                                                 uint64_t max_chunks, uint64_t* chunk_sum,
                                                                 const uint64_t* __restrict__ chunk_pos,
                                                                 const uint64_t* __restrict__ val_pos, uint8_t* out) {
  __shared__ uint32_t wsum[kEncThreads / 64];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
  const uint64_t total = min(chunk_base[count], max_chunks);
  for (uint64_t c = blockIdx.x; c < total; c += gridDim.x) {
    uint64_t lo = 0, hi = count;  // the last record whose first chunk is <= c: records without chunks share a base
    while (hi - lo > 1) {
      const uint64_t mid = (lo + hi) >> 1;
      if (chunk_base[mid] <= c) lo = mid; else hi = mid;
    }
    const uint64_t i = lo, st = start[i], e = st + len[i];
    const uint64_t A = st & ~uint64_t(15), E16 = (e + 15) & ~uint64_t(15);
    const uint64_t cb = A + (c - chunk_base[i]) * kLongChunk, ce = min(cb + kLongChunk, E16);
    uint64_t obase = 0;
    if (WRITE) {
      const uint64_t vp = val_pos[i];
      if (vp == kNoPos) continue;  // the line lies past out_cap (workgroup-uniform)
      obase = vp + (chunk_pos[c] - chunk_pos[chunk_base[i]]);
    }
    uint32_t mine = 0;  // WRITE = false: this lane's widths over all steps
    for (uint64_t it = cb; it < ce; it += kLongStep) {
      const uint64_t blk = it + 16u * tid;
      uint32_t by32[6] = {0, 0, 0, 0, 0, 0};
      uint32_t sum = 0;
      uint64_t widths = 0;  // 4 bits per byte
      bool plain = false;
      if (blk < ce) {
        const uint4 q = *reinterpret_cast<const uint4*>(data + blk);
        by32[1] = q.x; by32[2] = q.y; by32[3] = q.z; by32[4] = q.w;
        if (blk >= st && blk + 16 <= e && ((special_bytes(q.x) | special_bytes(q.y) | special_bytes(q.z) | special_bytes(q.w)) == 0u)) {
          plain = true;  // ASCII with nothing to escape: every width is 1, whatever the neighbours
          sum = 16;
        } else {
          if (blk > A) by32[0] = *reinterpret_cast<const uint32_t*>(data + blk - 4);
          if (blk + 16 < E16) by32[5] = *reinterpret_cast<const uint32_t*>(data + blk + 16);
          uint8_t by[24];
#pragma unroll
          for (int k = 0; k < 24; ++k) by[k] = uint8_t(by32[k >> 2] >> (8 * (k & 3)));
#pragma unroll
          for (int k = 0; k < 16; ++k) {
            const uint64_t p = blk + uint64_t(k);
            if (p < st || p >= e) continue;
            const uint32_t before = uint32_t(min(p - st, uint64_t(3))), after = uint32_t(min(e - 1 - p, uint64_t(3)));
            const uint32_t wd = escape_width(by + k + 1, before, after);
            sum += wd;
            widths |= uint64_t(wd) << (4 * k);
          }
        }
      }
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
      for (uint32_t k = 0; k < kEncThreads / 64; ++k) {
        if (k < wv) before_me += wsum[k];
        step_total += wsum[k];
      }
      __syncthreads();  // wsum is rewritten next step
      if (blk < ce) {
        uint8_t* o = out + obase + before_me;
        if (plain) {
#pragma unroll
          for (int k = 0; k < 16; ++k) o[k] = uint8_t(by32[1 + (k >> 2)] >> (8 * (k & 3)));
        } else {
          uint8_t by[24];
#pragma unroll
          for (int k = 0; k < 24; ++k) by[k] = uint8_t(by32[k >> 2] >> (8 * (k & 3)));
#pragma unroll
          for (int k = 0; k < 16; ++k) {
            const uint32_t wd = uint32_t(widths >> (4 * k)) & 15u;
            if (wd == 0) continue;  // outside the value, or swallowed
            const uint64_t p = blk + uint64_t(k);
            escape_put(by + k + 1, uint32_t(min(e - 1 - p, uint64_t(3))), wd, o);
            o += wd;
          }
        }
      }
      obase += step_total;
    }
    if (!WRITE) {
      const uint32_t inc = wave_inclusive(mine, lane);
      if (lane == 63) wsum[wv] = inc;
      __syncthreads();
      if (tid == 0) {
        uint64_t t = 0;
        for (uint32_t k = 0; k < kEncThreads / 64; ++k) t += wsum[k];
        chunk_sum[c] = t;
      }
      __syncthreads();
    }
  }
}

// a long value's encoded length, from its chunks' sums, into its line's length
__global__ __launch_bounds__(kEncThreads) void long_fix_kernel(const uint64_t* len, uint64_t count,
                                                               const uint64_t* nchunks, const uint64_t* chunk_base,
                                                               const uint64_t* chunk_pos, uint64_t max_chunks,
                                                               uint64_t* enc_len) {
  for (uint64_t i = uint64_t(blockIdx.x) * kEncThreads + threadIdx.x; i < count; i += uint64_t(gridDim.x) * kEncThreads) {
    if (nchunks[i] == 0) continue;
    const uint64_t c0 = min(chunk_base[i], max_chunks), c1 = min(chunk_base[i + 1], max_chunks);
    enc_len[i] += (chunk_pos[c1] - chunk_pos[c0]) - len[i];
  }
}

__global__ __launch_bounds__(kEncThreads) void gather_len_kernel(const uint32_t* idx, const uint64_t* enc_len,
                                                                 uint64_t* len_sorted, uint64_t count) {
  for (uint64_t j = uint64_t(blockIdx.x) * kEncThreads + threadIdx.x; j < count; j += uint64_t(gridDim.x) * kEncThreads)
    len_sorted[j] = enc_len[idx[j]];
}

// bounds[p] / bounds[nreduce + p]: byte range of partition p (both 0 when
// empty; zeroed beforehand); bounds[2 * nreduce]: total bytes
__global__ __launch_bounds__(kEncThreads) void bounds_kernel(const uint16_t* part, const uint64_t* pos,
                                                             const uint64_t* len_sorted, uint64_t count,
                                                             uint32_t nreduce, uint64_t* bounds) {
  for (uint64_t j = uint64_t(blockIdx.x) * kEncThreads + threadIdx.x; j < count; j += uint64_t(gridDim.x) * kEncThreads) {
    const uint32_t p = part[j];
    if (j == 0 || part[j - 1] != p) bounds[p] = pos[j];
    if (j + 1 == count || part[j + 1] != p) bounds[nreduce + p] = pos[j] + len_sorted[j];
    if (j + 1 == count) bounds[2 * nreduce] = pos[j] + len_sorted[j];
  }
}

// Per-thread writer of one record's line (values that need escaping). A long
// value's bytes are left to the chunk pass: its place goes to val_pos[i].
__device__ void write_line_thread(const WindowEncodeArgs& wa, uint64_t i, uint8_t* out, uint64_t P, uint64_t enc,
                                  bool is_long, uint64_t* val_pos) {
  const EncodeArgs& a = wa.e;
  uint8_t* o = out + P;
  put_str(o, "{\"Key\":\"");
  for (uint32_t k = 0; k < a.fname_json_len; ++k) *o++ = a.fname_json[k];
  put_str(o, " (line number #");
  uint8_t d[20];
  const uint32_t nd = digits_of(wa.line_base + a.line_no[i], d);
  for (uint32_t k = 0; k < nd; ++k) *o++ = uint8_t('0' + d[k]);
  put_str(o, ")\",\"Value\":\"");
  const uint64_t L = a.len[i], around = kFixedBytes + a.fname_json_len + nd;
  if (is_long) {
    val_pos[i] = uint64_t(o - out);
    o += enc - around;
  } else if (enc == around + L) {
    copy_bytes(o, a.data + a.start[i], L);
    o += L;
  } else {
    o += json_body<true>(a.data + a.start[i], L, o);
  }
  put_str(o, "\"}\n");
}

// encode_write_kernel (encode.hip) with the stream's line_base in the digits and
// the long values' bodies left out: one WAVE per 64 output lines.
constexpr uint32_t kHeadMax = 2048;
constexpr int kEncWaves = kEncThreads / 64;
__global__ __launch_bounds__(kEncThreads) void win_write_kernel(WindowEncodeArgs wa, const uint32_t* idx,
                                                                const uint64_t* pos, const uint64_t* len_sorted,
                                                                const uint64_t* nchunks, uint64_t* val_pos,
                                                                uint8_t* out, uint64_t out_cap) {
  const EncodeArgs& a = wa.e;
  __shared__ uint8_t head[kHeadMax];
  __shared__ uint8_t dig[kEncWaves][64][20];
  const uint32_t F = a.fname_json_len, A = 8u + F + 15u;  // head bytes (host guarantees A <= kHeadMax)
  for (uint32_t k = threadIdx.x; k < A; k += kEncThreads)
    head[k] = k < 8u ? uint8_t("{\"Key\":\""[k]) : k < 8u + F ? a.fname_json[k - 8u] : uint8_t(" (line number #"[k - 8u - F]);
  __syncthreads();
  const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
  const uint64_t nwaves = uint64_t(gridDim.x) * kEncWaves;
  for (uint64_t j0 = (uint64_t(blockIdx.x) * kEncWaves + wv) * 64u; j0 < a.count; j0 += nwaves * 64u) {
    const uint64_t jm = j0 + lane;
    uint64_t P = 0, T = 0, st = 0, L = 0, i = 0;
    uint32_t nd = 0;
    bool is_long = false;
    if (jm < a.count) {
      i = idx[jm];
      P = pos[jm];
      T = len_sorted[jm];
      st = a.start[i];
      L = a.len[i];
      is_long = nchunks[i] != 0;
      uint8_t d[20];
      nd = digits_of(wa.line_base + a.line_no[i], d);
      for (uint32_t k = 0; k < nd; ++k) dig[wv][lane][k] = d[k];
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const uint32_t cnt = uint32_t(min(uint64_t(64), a.count - j0));
    for (uint32_t r = 0; r < cnt; ++r) {
      const uint64_t Pr = __shfl(P, int(r), 64), Tr = __shfl(T, int(r), 64);
      const uint64_t str = __shfl(st, int(r), 64), Lr = __shfl(L, int(r), 64);
      const uint32_t ndr = uint32_t(__shfl(int(nd), int(r), 64));
      const bool long_r = __shfl(int(is_long), int(r), 64) != 0;
      if (Pr + Tr > out_cap) {
        if (lane == r && is_long) val_pos[i] = kNoPos;
        continue;
      }
      // escaped value: wave-uniform, rare. A long one may keep its length (valid
      // UTF-8 only); the chunk pass writes it all the same and needs its place.
      if (long_r || Tr != kFixedBytes + F + ndr + Lr) {
        if (lane == r) write_line_thread(wa, i, out, P, T, is_long, val_pos);
        continue;
      }
      const uint64_t V0 = uint64_t(A) + ndr + 12u;  // line offset of the first value byte
      const uint64_t d0 = Pr >> 2, d1 = (Pr + Tr + 3) >> 2;
      for (uint64_t d = d0 + lane; d < d1; d += 64) {
        const uint64_t q0 = 4u * d;
        const int64_t o0 = int64_t(q0) - int64_t(Pr);  // line offset of the dword's byte 0
        const uint64_t src = str + uint64_t(o0 - int64_t(V0));  // buffer position of byte 0 if it were value
        if (o0 >= int64_t(V0) && uint64_t(o0) + 4u <= V0 + Lr && ((src + 3) | 3u) < a.n) {
          const uint32_t sh = uint32_t(src & 3u);
          const uint32_t* w = reinterpret_cast<const uint32_t*>(a.data + (src & ~uint64_t(3)));
          const uint32_t lo = w[0], hi = sh ? w[1] : 0u;
          *reinterpret_cast<uint32_t*>(out + q0) = __builtin_amdgcn_alignbyte(hi, lo, sh);
          continue;
        }
        uint32_t word = 0, have = 0;
#pragma unroll
        for (uint32_t b = 0; b < 4; ++b) {
          const int64_t ob = o0 + int64_t(b);
          if (ob < 0 || uint64_t(ob) >= Tr) continue;
          const uint64_t o = uint64_t(ob);
          uint32_t ch;
          if (o < A) ch = head[o];
          else if (o < uint64_t(A) + ndr) ch = uint32_t('0') + dig[wv][r][o - A];
          else if (o < V0) ch = uint8_t(")\",\"Value\":\""[o - A - ndr]);
          else if (o < V0 + Lr) ch = a.data[str + (o - V0)];
          else ch = uint8_t("\"}\n"[o - V0 - Lr]);
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
    __builtin_amdgcn_wave_barrier();  // the LDS digit row is rewritten next round
  }
}

// the per-thread writer for file names whose head does not fit kHeadMax
__global__ __launch_bounds__(kEncThreads) void win_write_thread_kernel(WindowEncodeArgs wa, const uint32_t* idx,
                                                                       const uint64_t* pos, const uint64_t* len_sorted,
                                                                       const uint64_t* nchunks, uint64_t* val_pos,
                                                                       uint8_t* out, uint64_t out_cap) {
  for (uint64_t j = uint64_t(blockIdx.x) * kEncThreads + threadIdx.x; j < wa.e.count;
       j += uint64_t(gridDim.x) * kEncThreads) {
    const uint64_t i = idx[j];
    const bool is_long = nchunks[i] != 0;
    if (pos[j] + len_sorted[j] > out_cap) {
      if (is_long) val_pos[i] = kNoPos;
      continue;
    }
    write_line_thread(wa, i, out, pos[j], len_sorted[j], is_long, val_pos);
  }
}

struct NonZero {
  __host__ __device__ uint64_t operator()(uint64_t x) const { return x != 0 ? 1u : 0u; }
};

inline size_t align256(size_t x) { return (x + 255) & ~size_t(255); }
inline int grid_for(uint64_t n) { return int(std::min<uint64_t>((n + kEncThreads - 1) / kEncThreads, 8192)); }
inline int wave_grid_for(uint64_t n) { return int(std::min<uint64_t>((n + 3) / 4, 16384)); }
inline int wave64_grid_for(uint64_t n) { return int(std::min<uint64_t>((n + 255) / 256, 4096)); }
}  // namespace

hipError_t encode_window_partitions(const WindowEncodeArgs& wa, void* scratch, size_t* scratch_bytes, uint8_t* out,
                                    uint64_t out_cap, uint64_t* d_bounds, hipStream_t s) {
  const EncodeArgs& a = wa.e;
  const uint64_t n = a.count;
  // Every long value has at least long_value bytes and at most len / kLongChunk
  // + 2 chunks (its first and last blocks may be partial), and the values lie
  // apart in the window: the chunks number at most max_chunks.
  const uint64_t lv = std::max<uint32_t>(wa.long_value, 1);
  const uint64_t max_chunks = a.n / kLongChunk + 2 * std::min<uint64_t>(n, a.n / lv) + 2;
  int end_bit = 1;
  while ((1u << end_bit) < a.nreduce) ++end_bit;
  size_t sort_tmp = 0, scan_tmp = 0, scan2_tmp = 0, scan3_tmp = 0, red_tmp = 0;
  hipError_t e = hipcub::DeviceRadixSort::SortPairs(nullptr, sort_tmp, (uint16_t*)nullptr, (uint16_t*)nullptr,
                                                    (uint32_t*)nullptr, (uint32_t*)nullptr, n, 0, end_bit, s);
  if (e != hipSuccess) return e;
  e = hipcub::DeviceScan::ExclusiveSum(nullptr, scan_tmp, (uint64_t*)nullptr, (uint64_t*)nullptr, n, s);
  if (e != hipSuccess) return e;
  e = hipcub::DeviceScan::ExclusiveSum(nullptr, scan2_tmp, (uint64_t*)nullptr, (uint64_t*)nullptr, n + 1, s);
  if (e != hipSuccess) return e;
  e = hipcub::DeviceScan::ExclusiveSum(nullptr, scan3_tmp, (uint64_t*)nullptr, (uint64_t*)nullptr, max_chunks + 1, s);
  if (e != hipSuccess) return e;
  hipcub::TransformInputIterator<uint64_t, NonZero, const uint64_t*> flags0(nullptr, NonZero());
  e = hipcub::DeviceReduce::Sum(nullptr, red_tmp, flags0, (uint64_t*)nullptr, n, s);
  if (e != hipSuccess) return e;
  const size_t tmp = std::max(std::max(sort_tmp, scan_tmp), std::max(std::max(scan2_tmp, scan3_tmp), red_tmp));
  const size_t need = 2 * align256(n * 2) + 2 * align256(n * 4) + 3 * align256(n * 8) + 2 * align256((n + 1) * 8) +
                      2 * align256((max_chunks + 1) * 8) + align256(tmp);
  if (!scratch || *scratch_bytes < need) {
    *scratch_bytes = need;
    return hipSuccess;
  }
  uint8_t* p = static_cast<uint8_t*>(scratch);
  auto take = [&](size_t bytes) {
    uint8_t* q = p;
    p += align256(bytes);
    return q;
  };
  uint16_t* part_in = reinterpret_cast<uint16_t*>(take(n * 2));
  uint16_t* part_out = reinterpret_cast<uint16_t*>(take(n * 2));
  uint32_t* idx_in = reinterpret_cast<uint32_t*>(take(n * 4));
  uint32_t* idx_out = reinterpret_cast<uint32_t*>(take(n * 4));
  uint64_t* enc_len = reinterpret_cast<uint64_t*>(take(n * 8));
  uint64_t* len_sorted = reinterpret_cast<uint64_t*>(take(n * 8));
  uint64_t* pos = reinterpret_cast<uint64_t*>(take(n * 8));
  uint64_t* nchunks = reinterpret_cast<uint64_t*>(take((n + 1) * 8));
  uint64_t* chunk_base = reinterpret_cast<uint64_t*>(take((n + 1) * 8));
  uint64_t* chunk_sum = reinterpret_cast<uint64_t*>(take((max_chunks + 1) * 8));
  uint64_t* chunk_pos = reinterpret_cast<uint64_t*>(take((max_chunks + 1) * 8));
  void* t = take(tmp);
  uint64_t* val_pos = enc_len;  // enc_len is dead once gathered into len_sorted

  e = hipMemsetAsync(d_bounds, 0, (2 * size_t(a.nreduce) + 2) * 8, s);
  if (e != hipSuccess || n == 0) return e;
  const int long_grid = int(std::min<uint64_t>(max_chunks, 4096));
  hipLaunchKernelGGL(win_measure_kernel, dim3(grid_for(n)), dim3(kEncThreads), 0, s, wa, part_in, idx_in, enc_len,
                     nchunks);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipLaunchKernelGGL(win_values_kernel, dim3(wave_grid_for(n)), dim3(kEncThreads), 0, s, wa, enc_len, nchunks);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  // the long values: chunk counts -> chunk ranges -> chunk sums -> offsets and lengths
  size_t tb = tmp;
  if ((e = hipcub::DeviceScan::ExclusiveSum(t, tb, nchunks, chunk_base, n + 1, s)) != hipSuccess) return e;
  if ((e = hipMemsetAsync(chunk_sum, 0, (max_chunks + 1) * 8, s)) != hipSuccess) return e;
  hipLaunchKernelGGL(long_chunk_kernel<false>, dim3(long_grid), dim3(kEncThreads), 0, s, a.data, a.start, a.len, n,
                     chunk_base, max_chunks, chunk_sum, nullptr, nullptr, nullptr);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  tb = tmp;
  if ((e = hipcub::DeviceScan::ExclusiveSum(t, tb, chunk_sum, chunk_pos, max_chunks + 1, s)) != hipSuccess) return e;
  hipLaunchKernelGGL(long_fix_kernel, dim3(grid_for(n)), dim3(kEncThreads), 0, s, a.len, n, nchunks, chunk_base,
                     chunk_pos, max_chunks, enc_len);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipcub::TransformInputIterator<uint64_t, NonZero, const uint64_t*> flags(nchunks, NonZero());
  tb = tmp;
  if ((e = hipcub::DeviceReduce::Sum(t, tb, flags, d_bounds + 2 * size_t(a.nreduce) + 1, n, s)) != hipSuccess) return e;
  // encode.hip's pipeline from here
  tb = tmp;
  if ((e = hipcub::DeviceRadixSort::SortPairs(t, tb, part_in, part_out, idx_in, idx_out, n, 0, end_bit, s)) !=
      hipSuccess)
    return e;
  hipLaunchKernelGGL(gather_len_kernel, dim3(grid_for(n)), dim3(kEncThreads), 0, s, idx_out, enc_len, len_sorted, n);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  tb = tmp;
  if ((e = hipcub::DeviceScan::ExclusiveSum(t, tb, len_sorted, pos, n, s)) != hipSuccess) return e;
  hipLaunchKernelGGL(bounds_kernel, dim3(grid_for(n)), dim3(kEncThreads), 0, s, part_out, pos, len_sorted, n,
                     a.nreduce, d_bounds);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if (8u + a.fname_json_len + 15u <= kHeadMax)
    hipLaunchKernelGGL(win_write_kernel, dim3(wave64_grid_for(n)), dim3(kEncThreads), 0, s, wa, idx_out, pos,
                       len_sorted, nchunks, val_pos, out, out_cap);
  else
    hipLaunchKernelGGL(win_write_thread_kernel, dim3(grid_for(n)), dim3(kEncThreads), 0, s, wa, idx_out, pos,
                       len_sorted, nchunks, val_pos, out, out_cap);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipLaunchKernelGGL(long_chunk_kernel<true>, dim3(long_grid), dim3(kEncThreads), 0, s, a.data, a.start, a.len, n,
                     chunk_base, max_chunks, nullptr, chunk_pos, val_pos, out);
  return hipGetLastError();
}

}  // namespace dgrep
