// batch.hip — per-split rebasing of one scan over many packed splits (batch.h).
//
// split_newlines_kernel streams P once and counts its '\n' per region; a
// two-kernel exclusive scan turns the counts into each split's first line.
// split_ranges_kernel and rebase_records_kernel then turn the scan's P-wide
// records into per-split ones. None of them touches the scan kernels.
#include "batch.h"

#include <algorithm>

namespace dgrep {

namespace {

constexpr int kThreads = 256;                              // 4 waves
constexpr int kPieces = 4;                                 // 16-B loads per lane and tile
constexpr uint64_t kRow = 64 * 16;                         // one wave's load: 1 KiB
constexpr uint64_t kTile = uint64_t(kThreads) * 16 * kPieces;  // 16 KiB per workgroup step

// bit 7 of byte j set iff byte j of w is '\n' (exact SWAR zero test of w ^ "\n\n\n\n")
__device__ __forceinline__ uint32_t nl_bits(uint32_t w) {
  const uint32_t x = w ^ 0x0a0a0a0au;
  const uint32_t t = (x & 0x7f7f7f7fu) + 0x7f7f7f7fu;
  return ~(t | x) & 0x80808080u;
}
__device__ __forceinline__ uint32_t nl_count(const uint4& v) {
  return __popc(nl_bits(v.x)) + __popc(nl_bits(v.y)) + __popc(nl_bits(v.z)) + __popc(nl_bits(v.w));
}

// Sum over the wave's 64 lanes (all active), every lane gets it. DPP: quads,
// half rows, rows, then row 0 -> 1 and 2 -> 3 (row_bcast15), rows 0-1 -> 2-3
// (row_bcast31); lane 63 ends with the total.
__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
  v += uint32_t(__builtin_amdgcn_update_dpp(0, int(v), 0xB1, 0xF, 0xF, false));   // quad_perm [1,0,3,2]
  v += uint32_t(__builtin_amdgcn_update_dpp(0, int(v), 0x4E, 0xF, 0xF, false));   // quad_perm [2,3,0,1]
  v += uint32_t(__builtin_amdgcn_update_dpp(0, int(v), 0x141, 0xF, 0xF, false));  // row_half_mirror
  v += uint32_t(__builtin_amdgcn_update_dpp(0, int(v), 0x140, 0xF, 0xF, false));  // row_mirror
  v += uint32_t(__builtin_amdgcn_update_dpp(0, int(v), 0x142, 0xA, 0xF, false));  // row_bcast15 into rows 1, 3
  v += uint32_t(__builtin_amdgcn_update_dpp(0, int(v), 0x143, 0xC, 0xF, false));  // row_bcast31 into rows 2, 3
  return uint32_t(__builtin_amdgcn_readlane(int(v), 63));
}

__device__ __forceinline__ unsigned long long wave_sum64(unsigned long long v) {
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
  return v;
}

// the last i in [lo, hi] with begin[i] <= pos (the caller knows begin[lo] <= pos)
__device__ __forceinline__ uint64_t find_split(const uint64_t* __restrict__ begin, uint64_t lo, uint64_t hi,
                                               uint64_t pos) {
  while (lo < hi) {
    const uint64_t mid = lo + (hi - lo + 1) / 2;
    if (begin[mid] <= pos) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

// the workgroup's `acc` summed into *dst (one atomic); every thread calls it
__device__ __forceinline__ void block_flush(uint32_t acc, unsigned long long* dst, uint32_t* part) {
  const uint32_t w = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = w;
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned long long s = (unsigned long long)part[0] + part[1] + part[2] + part[3];
    if (s) atomicAdd(dst, s);
  }
  __syncthreads();
}

// Cold path: one wave's 1 KiB row [row_start, row_start + kRow) of a tile that
// is not inside one region; lane l holds the 16 bytes at row_start + 16 l in v.
// `cur` = a split at or before the row's. The row, then the lane's piece, then
// its bytes are attributed to their regions, from the registers alone.
__device__ __forceinline__ void cold_row(const BatchArgs& a, uint64_t cur, uint64_t row_start, const uint4& v) {
  if (row_start >= a.n) return;  // wave-uniform
  const uint64_t row_end = min(row_start + kRow, a.n);
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t pos = row_start + 16u * lane;
  uint32_t w[4] = {v.x, v.y, v.z, v.w};
  if (pos + 16 > a.n) {
    // P's last piece: bytes at or past n become 0 (not '\n')
    const uint32_t valid = pos < a.n ? uint32_t(a.n - pos) : 0u;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const uint32_t keep = valid > 4u * j ? min(valid - 4u * j, 4u) : 0u;
      w[j] &= keep >= 4u ? 0xffffffffu : (1u << (8u * keep)) - 1u;
    }
  }
  const uint32_t c = __popc(nl_bits(w[0])) + __popc(nl_bits(w[1])) + __popc(nl_bits(w[2])) + __popc(nl_bits(w[3]));
  const uint64_t s0 = find_split(a.begin, cur, a.k - 1, row_start);
  if (row_end <= a.begin[s0 + 1]) {  // wave-uniform: the whole row lies in region s0
    const uint32_t total = wave_sum(c);
    if (lane == 0 && total) atomicAdd(&a.lines[s0], (unsigned long long)total);
    return;
  }
  const uint64_t s1 = find_split(a.begin, s0, a.k - 1, row_end - 1);
  if (pos >= a.n) return;
  const uint64_t pend = min(pos + 16, a.n);
  uint64_t s = find_split(a.begin, s0, s1, pos);
  uint64_t e = a.begin[s + 1];
  if (pend <= e) {  // the piece lies in region s
    if (c) atomicAdd(&a.lines[s], (unsigned long long)c);
    return;
  }
  // region boundaries inside the piece: byte by byte, one add per region
  uint32_t run = 0;
#pragma unroll
  for (int b = 0; b < 16; ++b) {
    const uint64_t q = pos + b;
    if (q < pend) {
      while (q >= e) {  // begin[k] = n + 1 > q ends it with s <= k - 1
        if (run) atomicAdd(&a.lines[s], (unsigned long long)run);
        run = 0;
        ++s;
        e = a.begin[s + 1];
      }
      run += ((w[b >> 2] >> (8 * (b & 3))) & 0xffu) == 0x0au ? 1u : 0u;
    }
  }
  if (run) atomicAdd(&a.lines[s], (unsigned long long)run);
}

// Workgroup b streams tiles [b, b + 1) * tiles_per_block of P, each lane four
// aligned 16-B loads per tile. While its tiles stay inside one region the
// counts stay in registers; they are flushed (wave reduction, one 64-bit
// atomic) when a tile meets a region boundary and at the end. Such a tile is
// attributed row by row from the registers it was loaded into (cold_row), so
// every byte is read once. Per-thread counts are u32: a thread sees 64 bytes
// per tile, so they hold for any P below 2^32 * 64 * threads bytes per grid.
__global__ __launch_bounds__(kThreads) void split_newlines_kernel(BatchArgs a, uint64_t tiles_per_block) {
  __shared__ uint32_t part[kThreads / 64];
  const uint64_t ntiles = (a.n + kTile - 1) / kTile;
  uint64_t t = uint64_t(blockIdx.x) * tiles_per_block;
  const uint64_t t_end = min(ntiles, t + tiles_per_block);
  if (t >= t_end) return;
  const uint4* __restrict__ p16 = reinterpret_cast<const uint4*>(a.data);
  uint64_t cur = find_split(a.begin, 0, a.k - 1, t * kTile);
  uint64_t cur_end = a.begin[cur + 1];
  uint32_t acc = 0;
  for (; t < t_end; ++t) {
    const uint64_t off = t * kTile;
    uint4 v[kPieces];
#pragma unroll
    for (int u = 0; u < kPieces; ++u) {
      const uint64_t pos = off + 16u * (uint64_t(u) * kThreads + threadIdx.x);
      v[u] = pos < a.n ? p16[pos >> 4] : make_uint4(0u, 0u, 0u, 0u);
    }
    if (off + kTile <= a.n && off + kTile <= cur_end) {  // a whole tile inside region cur
#pragma unroll
      for (int u = 0; u < kPieces; ++u) acc += nl_count(v[u]);
      continue;
    }
    block_flush(acc, &a.lines[cur], part);
    acc = 0;
#pragma unroll
    for (int u = 0; u < kPieces; ++u)
      cold_row(a, cur, off + 16u * (uint64_t(u) * kThreads + (threadIdx.x & ~63u)), v[u]);
    const uint64_t tile_end = min(off + kTile, a.n);
    cur = find_split(a.begin, cur, a.k - 1, tile_end);
    cur_end = a.begin[cur + 1];
  }
  block_flush(acc, &a.lines[cur], part);
}

// Exclusive scan over lines[0, k), in place, in two kernels: workgroup b owns
// the `chunk` entries from b * chunk. First their sum (and, one thread per
// split, the separator check); then each workgroup adds the sums before it and
// scans its entries 256 at a time.
__global__ __launch_bounds__(kThreads) void split_sums_kernel(BatchArgs a, uint64_t chunk) {
  __shared__ unsigned long long part[kThreads / 64];
  const uint64_t lo = uint64_t(blockIdx.x) * chunk, hi = min(a.k, lo + chunk);
  unsigned long long s = 0;
  for (uint64_t i = lo + threadIdx.x; i < hi; i += kThreads) {
    s += a.lines[i];
    if (i + 1 < a.k && a.data[a.begin[i + 1] - 1] != 0x0a) atomicMin(a.bad_split, (unsigned long long)i);
  }
  s = wave_sum64(s);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) a.block_sums[blockIdx.x] = part[0] + part[1] + part[2] + part[3];
}

__global__ __launch_bounds__(kThreads) void split_first_lines_kernel(BatchArgs a, uint64_t chunk) {
  __shared__ unsigned long long part[kThreads / 64];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  unsigned long long before = 0;
  for (uint32_t j = threadIdx.x; j < blockIdx.x; j += kThreads) before += a.block_sums[j];
  before = wave_sum64(before);
  if (lane == 0) part[wave] = before;
  __syncthreads();
  unsigned long long carry = part[0] + part[1] + part[2] + part[3];
  __syncthreads();
  const uint64_t lo = uint64_t(blockIdx.x) * chunk, hi = min(a.k, lo + chunk);
  for (uint64_t base = lo; base < hi; base += kThreads) {
    const uint64_t i = base + threadIdx.x;
    const unsigned long long x = i < hi ? a.lines[i] : 0ull;
    unsigned long long inc = x;  // inclusive scan within the wave
    for (int d = 1; d < 64; d <<= 1) {
      const unsigned long long o = __shfl_up(inc, d, 64);
      if (int(lane) >= d) inc += o;
    }
    if (lane == 63) part[wave] = inc;
    __syncthreads();
    unsigned long long wave_off = 0, total = 0;
#pragma unroll
    for (uint32_t j = 0; j < kThreads / 64; ++j) {
      const unsigned long long p = part[j];
      wave_off += j < wave ? p : 0ull;
      total += p;
    }
    if (i < hi) a.lines[i] = carry + wave_off + inc - x;
    carry += total;
    __syncthreads();
  }
}

// one thread per split (and one for the closing entry)
__global__ __launch_bounds__(kThreads) void split_ranges_kernel(BatchArgs a, const uint64_t* __restrict__ start,
                                                                uint64_t nrec, uint64_t* __restrict__ split_begin) {
  for (uint64_t s = uint64_t(blockIdx.x) * kThreads + threadIdx.x; s <= a.k; s += uint64_t(gridDim.x) * kThreads) {
    uint64_t lo = 0, hi = nrec;  // first record with start >= begin[s]
    if (s == a.k) lo = nrec;
    const uint64_t b = a.begin[s];
    while (lo < hi) {
      const uint64_t mid = lo + (hi - lo) / 2;
      if (start[mid] < b) lo = mid + 1;
      else hi = mid;
    }
    split_begin[s] = lo;
  }
}

// one thread per record. start == begin[i] belongs to split i (also when split
// i is empty: begin is strictly increasing), and an empty last line, at
// begin[i+1] - 1 (the separator's offset, or n for the last split), to split i.
__global__ __launch_bounds__(kThreads) void rebase_records_kernel(BatchArgs a, uint64_t* __restrict__ line_no,
                                                                  uint64_t* __restrict__ start,
                                                                  uint32_t* __restrict__ split, uint64_t nrec) {
  for (uint64_t r = uint64_t(blockIdx.x) * kThreads + threadIdx.x; r < nrec; r += uint64_t(gridDim.x) * kThreads) {
    const uint64_t st = start[r];
    const uint64_t s = find_split(a.begin, 0, a.k - 1, st);
    split[r] = uint32_t(s);
    line_no[r] -= a.lines[s];
    start[r] = st - a.begin[s];
  }
}

int grid_for(uint64_t items_per_thread_total, int num_cus) {
  const uint64_t blocks = (items_per_thread_total + kThreads - 1) / kThreads;
  return int(std::max<uint64_t>(1, std::min<uint64_t>(blocks, uint64_t(std::max(num_cus, 1)) * 8)));
}

}  // namespace

hipError_t batch_split_newlines(const BatchArgs& a, int num_cus, hipStream_t s) {
  if (a.n) {
    // 8 workgroups of 256 threads per CU keep every SIMD at 8 waves
    const uint64_t ntiles = (a.n + kTile - 1) / kTile;
    const uint64_t want = std::min<uint64_t>(ntiles, uint64_t(std::max(num_cus, 1)) * 8);
    const uint64_t tpb = (ntiles + want - 1) / want;
    const int grid = int((ntiles + tpb - 1) / tpb);
    hipLaunchKernelGGL(split_newlines_kernel, dim3(grid), dim3(kThreads), 0, s, a, tpb);
  }
  uint64_t blocks = std::min<uint64_t>((a.k + kThreads - 1) / kThreads, kBatchScanBlocks);
  const uint64_t chunk = (((a.k + blocks - 1) / blocks) + kThreads - 1) / kThreads * kThreads;
  blocks = (a.k + chunk - 1) / chunk;
  hipLaunchKernelGGL(split_sums_kernel, dim3(int(blocks)), dim3(kThreads), 0, s, a, chunk);
  hipLaunchKernelGGL(split_first_lines_kernel, dim3(int(blocks)), dim3(kThreads), 0, s, a, chunk);
  return hipGetLastError();
}

hipError_t batch_split_ranges(const BatchArgs& a, const uint64_t* start, uint64_t nrec, uint64_t* split_begin,
                              int num_cus, hipStream_t s) {
  hipLaunchKernelGGL(split_ranges_kernel, dim3(grid_for(a.k + 1, num_cus)), dim3(kThreads), 0, s, a, start, nrec,
                     split_begin);
  return hipGetLastError();
}

hipError_t batch_rebase(const BatchArgs& a, uint64_t* line_no, uint64_t* start, uint32_t* split, uint64_t nrec,
                        int num_cus, hipStream_t s) {
  if (nrec == 0) return hipSuccess;
  hipLaunchKernelGGL(rebase_records_kernel, dim3(grid_for(nrec, num_cus)), dim3(kThreads), 0, s, a, line_no, start,
                     split, nrec);
  return hipGetLastError();
}

}  // namespace dgrep
