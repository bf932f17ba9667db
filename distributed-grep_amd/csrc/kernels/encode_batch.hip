// encode_batch.hip — the partition + intermediate writer over a batch scan.
//
// encode.hip writes the nreduce files mr-<task>-<p> of ONE map task from the
// scan records of one split. A batch scan (batch.h) returns the records of k
// map tasks over one packed buffer P; this file writes all k * nreduce files
// in one pass over those records, with the pipeline of encode.hip generalised:
//   1. measure: per record, cell = split * nreduce + ihash(Key) % nreduce (the
//      FNV-1a state after "filename[split] (line number #" comes from a device
//      table, continued over the digits and ')') and the encoded line's length;
//      a wave-per-record pass corrects the length of values that need escaping;
//   2. a stable radix sort of (cell, record) over ceil(log2(cells)) bits keeps
//      line order inside a cell; an exclusive scan of the sorted lengths gives
//      each line's byte offset;
//   3. cell offsets: one thread per cell binary-searches the sorted cell ids,
//      so an empty cell gets its successor's offset with nothing to zero first;
//   4. write: one wave per 64 sorted lines. When the 64 lines belong to one
//      split (wave-uniform test; the common case for a split with more than a
//      few matches) the line head `{"Key":"<file> (line number #` is staged in
//      the wave's LDS row; otherwise, or when the head is longer than the row,
//      head bytes are read from the filename table in global memory (small,
//      L2-resident). File names of any length are written by the same kernel.
// A record's value lies at P[begin[split] + start : + len).
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>

#include "encode_batch.h"
#include "encode_common.h"

namespace dgrep {

namespace {
constexpr int kEncThreads = 256;
constexpr int kEncWaves = kEncThreads / 64;
constexpr uint32_t kHeadRow = 2048;  // LDS bytes per wave for a staged head

__global__ __launch_bounds__(kEncThreads) void batch_measure_kernel(EncodeBatchArgs a, uint32_t* cell, uint32_t* idx,
                                                                    uint64_t* enc_len) {
  for (uint64_t i = uint64_t(blockIdx.x) * kEncThreads + threadIdx.x; i < a.count;
       i += uint64_t(gridDim.x) * kEncThreads) {
    const uint32_t sp = a.split[i];
    uint8_t d[20];
    const uint32_t nd = digits_of(a.line_no[i], d);
    uint32_t h = a.name_hash[sp];
    for (uint32_t k = 0; k < nd; ++k) h = fnv_step(h, uint32_t('0') + d[k]);
    h = fnv_step(h, uint32_t(')'));
    cell[i] = sp * a.nreduce + (h & 0x7fffffffu) % a.nreduce;  // < k * nreduce < 2^32
    idx[i] = uint32_t(i);
    enc_len[i] = kFixedBytes + (a.name_off[sp + 1] - a.name_off[sp]) + nd + a.len[i];
  }
}

// One WAVE per record, as encode_values_kernel: the value's bytes tested 4 per
// lane in aligned dwords of P; a value with anything to escape gets its exact
// encoded length from json_body (lane 0).
__global__ __launch_bounds__(kEncThreads) void batch_values_kernel(EncodeBatchArgs a, uint64_t* enc_len) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t waves = uint64_t(gridDim.x) * kEncWaves;
  for (uint64_t i = uint64_t(blockIdx.x) * kEncWaves + (threadIdx.x >> 6); i < a.count; i += waves) {
    const uint64_t st = a.begin[a.split[i]] + a.start[i], e = st + a.len[i];
    bool bad = false;
    for (uint64_t w = (st & ~uint64_t(3)) + 4u * lane; w < e; w += 256) {
      uint32_t x;
      if (w + 4 <= a.n) {
        x = *reinterpret_cast<const uint32_t*>(a.data + w);
      } else {  // P's last partial dword: no read past n
        x = 0x20202020u;
        for (uint32_t k = 0; w + k < a.n; ++k) x = (x & ~(0xffu << (8 * k))) | (uint32_t(a.data[w + k]) << (8 * k));
      }
      const uint32_t in = (w >= st && w + 4 <= e) ? 0x80808080u : range_mask(w, st, e);
      bad = bad || (special_bytes(x) & in) != 0u;
    }
    if (__ballot(bad) == 0ull) continue;  // wave-uniform: plain value
    if (lane == 0) enc_len[i] += json_body<false>(a.data + st, e - st, nullptr) - (e - st);
  }
}

__global__ __launch_bounds__(kEncThreads) void batch_gather_len_kernel(const uint32_t* idx, const uint64_t* enc_len,
                                                                       uint64_t* len_sorted, uint64_t count) {
  for (uint64_t j = uint64_t(blockIdx.x) * kEncThreads + threadIdx.x; j < count; j += uint64_t(gridDim.x) * kEncThreads)
    len_sorted[j] = enc_len[idx[j]];
}

// one thread per cell, and one for the closing entry (count >= 1):
// cell_off[c] = offset of the first sorted line whose cell is >= c, or the total
__global__ __launch_bounds__(kEncThreads) void batch_cell_off_kernel(const uint32_t* __restrict__ cell_sorted,
                                                                     const uint64_t* __restrict__ pos,
                                                                     const uint64_t* __restrict__ len_sorted,
                                                                     uint64_t count, uint64_t cells,
                                                                     uint64_t* __restrict__ cell_off) {
  const uint64_t total = pos[count - 1] + len_sorted[count - 1];
  for (uint64_t c = uint64_t(blockIdx.x) * kEncThreads + threadIdx.x; c <= cells; c += uint64_t(gridDim.x) * kEncThreads) {
    uint64_t lo = 0, hi = count;
    while (lo < hi) {
      const uint64_t mid = lo + (hi - lo) / 2;
      if (uint64_t(cell_sorted[mid]) < c) lo = mid + 1;
      else hi = mid;
    }
    cell_off[c] = lo < count ? pos[lo] : total;
  }
}

// Per-thread writer of one record's line (values that need escaping).
__device__ void write_line_thread(const uint8_t* name, uint32_t F, uint64_t line_no, const uint8_t* value, uint64_t L,
                                  uint8_t* o, uint64_t enc) {
  put_str(o, "{\"Key\":\"");
  for (uint32_t k = 0; k < F; ++k) *o++ = name[k];
  put_str(o, " (line number #");
  uint8_t d[20];
  const uint32_t nd = digits_of(line_no, d);
  for (uint32_t k = 0; k < nd; ++k) *o++ = uint8_t('0' + d[k]);
  put_str(o, ")\",\"Value\":\"");
  if (enc == kFixedBytes + F + nd + L) {
    copy_bytes(o, value, L);
    o += L;
  } else {
    o += json_body<true>(value, L, o);
  }
  put_str(o, "\"}\n");
}

// One WAVE per 64 output lines (sorted order j0 .. j0 + 63), as
// encode_write_kernel: lane l fetches line j0 + l's record and writes its line
// number's digits to the wave's LDS row; then the wave walks the 64 lines, each
// broadcast from its lane, and lane l builds the line's output dwords
// (pos >> 2) + l + 64k from its five pieces. The head differs per line here:
// it comes from the wave's LDS row when all the wave's lines share a split and
// the head fits the row (`staged`, wave-uniform), else from the filename table.
// Guards as in the single-split writer: a dword wholly inside the value is read
// as two aligned dwords of P only when the second one ends before P does; the
// first and last dwords of a line are stored byte by byte; a line that would
// end past out_cap is skipped.
__global__ __launch_bounds__(kEncThreads) void batch_write_kernel(EncodeBatchArgs a, const uint32_t* idx,
                                                                  const uint64_t* pos, const uint64_t* len_sorted,
                                                                  uint8_t* out, uint64_t out_cap) {
  __shared__ uint8_t head[kEncWaves][kHeadRow];
  __shared__ uint8_t dig[kEncWaves][64][20];
  const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
  const uint64_t nwaves = uint64_t(gridDim.x) * kEncWaves;
  for (uint64_t j0 = (uint64_t(blockIdx.x) * kEncWaves + wv) * 64u; j0 < a.count; j0 += nwaves * 64u) {
    const uint64_t jm = j0 + lane;
    uint64_t P = 0, T = 0, src = 0, L = 0, i = 0, no = 0;
    uint32_t nd = 0, F = 0, sp = 0;
    if (jm < a.count) {
      i = idx[jm];
      P = pos[jm];
      T = len_sorted[jm];
      sp = a.split[i];
      src = a.begin[sp] + a.start[i];
      L = a.len[i];
      no = a.name_off[sp];
      F = uint32_t(a.name_off[sp + 1] - no);
      uint8_t d[20];
      nd = digits_of(a.line_no[i], d);
      for (uint32_t k = 0; k < nd; ++k) dig[wv][lane][k] = d[k];
    }
    // lane 0 holds line j0 < count
    const uint32_t sp0 = uint32_t(__shfl(int(sp), 0, 64)), F0 = uint32_t(__shfl(int(F), 0, 64));
    const uint64_t no0 = __shfl(no, 0, 64);
    const bool staged = __ballot(jm < a.count && sp != sp0) == 0ull && 8u + F0 + 15u <= kHeadRow;
    if (staged) {
      for (uint32_t k = lane; k < 8u + F0 + 15u; k += 64u)
        head[wv][k] = k < 8u ? uint8_t("{\"Key\":\""[k])
                             : k < 8u + F0 ? a.names[no0 + (k - 8u)] : uint8_t(" (line number #"[k - 8u - F0]);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const uint32_t cnt = uint32_t(min(uint64_t(64), a.count - j0));
    for (uint32_t r = 0; r < cnt; ++r) {
      const uint64_t Pr = __shfl(P, int(r), 64), Tr = __shfl(T, int(r), 64);
      const uint64_t srcr = __shfl(src, int(r), 64), Lr = __shfl(L, int(r), 64);
      const uint64_t nor = __shfl(no, int(r), 64);
      const uint32_t ndr = uint32_t(__shfl(int(nd), int(r), 64)), Fr = uint32_t(__shfl(int(F), int(r), 64));
      if (Pr + Tr > out_cap) continue;
      if (Tr != kFixedBytes + Fr + ndr + Lr) {  // escaped value: wave-uniform, rare
        if (lane == r) write_line_thread(a.names + no, F, a.line_no[i], a.data + src, L, out + P, T);
        continue;
      }
      const uint32_t A = 8u + Fr + 15u;                 // head bytes
      const uint64_t V0 = uint64_t(A) + ndr + 12u;      // line offset of the first value byte
      const uint64_t d0 = Pr >> 2, d1 = (Pr + Tr + 3) >> 2;
      for (uint64_t d = d0 + lane; d < d1; d += 64) {
        const uint64_t q0 = 4u * d;
        const int64_t o0 = int64_t(q0) - int64_t(Pr);  // line offset of the dword's byte 0
        const uint64_t s0 = srcr + uint64_t(o0 - int64_t(V0));  // P position of byte 0 if it were value
        if (o0 >= int64_t(V0) && uint64_t(o0) + 4u <= V0 + Lr && ((s0 + 3) | 3u) < a.n) {
          const uint32_t sh = uint32_t(s0 & 3u);
          const uint32_t* w = reinterpret_cast<const uint32_t*>(a.data + (s0 & ~uint64_t(3)));
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
          if (o < A) {
            if (staged) ch = head[wv][o];
            else if (o < 8u) ch = uint8_t("{\"Key\":\""[o]);
            else if (o < 8u + Fr) ch = a.names[nor + (o - 8u)];
            else ch = uint8_t(" (line number #"[o - 8u - Fr]);
          }
          else if (o < uint64_t(A) + ndr) ch = uint32_t('0') + dig[wv][r][o - A];
          else if (o < V0) ch = uint8_t(")\",\"Value\":\""[o - A - ndr]);
          else if (o < V0 + Lr) ch = a.data[srcr + (o - V0)];
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
    __builtin_amdgcn_wave_barrier();  // the LDS rows are rewritten next round
  }
}

inline size_t align256(size_t x) { return (x + 255) & ~size_t(255); }
inline int grid_for(uint64_t n) { return int(std::min<uint64_t>((n + kEncThreads - 1) / kEncThreads, 8192)); }
// one wave per record: 4 records per workgroup
inline int wave_grid_for(uint64_t n) { return int(std::min<uint64_t>((n + 3) / 4, 16384)); }
// one wave per 64 records
inline int wave64_grid_for(uint64_t n) { return int(std::min<uint64_t>((n + 255) / 256, 4096)); }
}  // namespace

hipError_t encode_batch(const EncodeBatchArgs& a, void* scratch, size_t* scratch_bytes, uint8_t* out,
                        uint64_t out_cap, uint64_t* d_cell_off, hipStream_t s) {
  const uint64_t n = a.count, cells = a.k * uint64_t(a.nreduce);
  int end_bit = 1;
  while ((1ull << end_bit) < cells) ++end_bit;
  size_t sort_tmp = 0, scan_tmp = 0;
  hipError_t e = hipcub::DeviceRadixSort::SortPairs(nullptr, sort_tmp, (uint32_t*)nullptr, (uint32_t*)nullptr,
                                                    (uint32_t*)nullptr, (uint32_t*)nullptr, n, 0, end_bit, s);
  if (e != hipSuccess) return e;
  e = hipcub::DeviceScan::ExclusiveSum(nullptr, scan_tmp, (uint64_t*)nullptr, (uint64_t*)nullptr, n, s);
  if (e != hipSuccess) return e;
  const size_t tmp = std::max(sort_tmp, scan_tmp);
  const size_t need = 4 * align256(n * 4) + 3 * align256(n * 8) + align256(tmp);
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
  uint32_t* cell_in = reinterpret_cast<uint32_t*>(take(n * 4));
  uint32_t* cell_out = reinterpret_cast<uint32_t*>(take(n * 4));
  uint32_t* idx_in = reinterpret_cast<uint32_t*>(take(n * 4));
  uint32_t* idx_out = reinterpret_cast<uint32_t*>(take(n * 4));
  uint64_t* enc_len = reinterpret_cast<uint64_t*>(take(n * 8));
  uint64_t* len_sorted = reinterpret_cast<uint64_t*>(take(n * 8));
  uint64_t* pos = reinterpret_cast<uint64_t*>(take(n * 8));
  void* t = take(tmp);

  if (n == 0) return hipMemsetAsync(d_cell_off, 0, (cells + 1) * 8, s);
  hipLaunchKernelGGL(batch_measure_kernel, dim3(grid_for(n)), dim3(kEncThreads), 0, s, a, cell_in, idx_in, enc_len);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipLaunchKernelGGL(batch_values_kernel, dim3(wave_grid_for(n)), dim3(kEncThreads), 0, s, a, enc_len);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  size_t tb = tmp;
  if ((e = hipcub::DeviceRadixSort::SortPairs(t, tb, cell_in, cell_out, idx_in, idx_out, n, 0, end_bit, s)) !=
      hipSuccess)
    return e;
  hipLaunchKernelGGL(batch_gather_len_kernel, dim3(grid_for(n)), dim3(kEncThreads), 0, s, idx_out, enc_len,
                     len_sorted, n);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  tb = tmp;
  if ((e = hipcub::DeviceScan::ExclusiveSum(t, tb, len_sorted, pos, n, s)) != hipSuccess) return e;
  hipLaunchKernelGGL(batch_cell_off_kernel, dim3(grid_for(cells + 1)), dim3(kEncThreads), 0, s, cell_out, pos,
                     len_sorted, n, cells, d_cell_off);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipLaunchKernelGGL(batch_write_kernel, dim3(wave64_grid_for(n)), dim3(kEncThreads), 0, s, a, idx_out, pos,
                     len_sorted, out, out_cap);
  return hipGetLastError();
}

}  // namespace dgrep
