// window.hip — the cut, the rebase and the value gather of a windowed scan (window.h).
//
// cut_kernel streams the window's bytes once and leaves, per workgroup, its
// '\n' count, the last '\n' it saw and the first one behind the carried tail;
// cut_finish_kernel folds those.
// rebase_append_kernel moves one window's records to the stream's coordinates
// at the running offset of the call's result arrays. The gather writes the
// matching lines' bytes back to back: an inclusive scan of the lengths, then
// one thread per short line and one wave per long one. None of them touches
// the scan kernels.
#include "window.h"

#include <hipcub/hipcub.hpp>

#include <algorithm>

namespace dgrep {

namespace {

constexpr int kThreads = 256;                                  // 4 waves
constexpr int kPieces = 4;                                     // 16-B loads per lane and tile
constexpr uint64_t kTile = uint64_t(kThreads) * 16 * kPieces;  // 16 KiB per workgroup step
constexpr uint64_t kShortLine = 64;                            // lines up to this many bytes: one thread each

// bit 7 of byte j set iff byte j of w is '\n' (exact SWAR zero test of w ^ "\n\n\n\n")
__device__ __forceinline__ uint32_t nl_bits(uint32_t w) {
  const uint32_t x = w ^ 0x0a0a0a0au;
  const uint32_t t = (x & 0x7f7f7f7fu) + 0x7f7f7f7fu;
  return ~(t | x) & 0x80808080u;
}

__device__ __forceinline__ unsigned long long wave_sum64(unsigned long long v) {
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
  return v;
}
__device__ __forceinline__ unsigned long long wave_max64(unsigned long long v) {
  for (int d = 32; d >= 1; d >>= 1) v = max(v, (unsigned long long)__shfl_xor(v, d, 64));
  return v;
}
__device__ __forceinline__ unsigned long long wave_min64(unsigned long long v) {
  for (int d = 32; d >= 1; d >>= 1) v = min(v, (unsigned long long)__shfl_xor(v, d, 64));
  return v;
}

// Workgroup b streams tiles [b, b + 1) * tiles_per_block, each lane four
// aligned 16-B loads per tile. A thread meets its pieces in ascending position,
// so the last '\n' it saw is the highest and the first one at or after `from`
// the lowest. partials[3 b] = the workgroup's '\n' count, [3 b + 1] = 1 + its
// last '\n' position (0: none), [3 b + 2] = its first '\n' position at or
// after `from` (kNoPos: none).
constexpr unsigned long long kNoPos = ~0ull;
__global__ __launch_bounds__(kThreads) void cut_kernel(const uint8_t* __restrict__ data, uint64_t n, uint64_t from,
                                                       uint64_t tiles_per_block,
                                                       unsigned long long* __restrict__ partials) {
  __shared__ unsigned long long part[3][kThreads / 64];
  const uint64_t ntiles = (n + kTile - 1) / kTile;
  uint64_t t = uint64_t(blockIdx.x) * tiles_per_block;
  const uint64_t t_end = min(ntiles, t + tiles_per_block);
  const uint4* __restrict__ p16 = reinterpret_cast<const uint4*>(data);
  unsigned long long acc = 0, last = 0, first = kNoPos;
  for (; t < t_end; ++t) {
    const uint64_t off = t * kTile;
    uint4 v[kPieces];
#pragma unroll
    for (int u = 0; u < kPieces; ++u) {
      const uint64_t pos = off + 16u * (uint64_t(u) * kThreads + threadIdx.x);
      v[u] = pos < n ? p16[pos >> 4] : make_uint4(0u, 0u, 0u, 0u);
    }
#pragma unroll
    for (int u = 0; u < kPieces; ++u) {
      const uint64_t pos = off + 16u * (uint64_t(u) * kThreads + threadIdx.x);
      uint32_t w[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
      if (pos + 16 > n) {
        // the last piece: bytes at or past n become 0 (not '\n')
        const uint32_t valid = pos < n ? uint32_t(n - pos) : 0u;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const uint32_t keep = valid > 4u * j ? min(valid - 4u * j, 4u) : 0u;
          w[j] &= keep >= 4u ? 0xffffffffu : (1u << (8u * keep)) - 1u;
        }
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const uint32_t b = nl_bits(w[j]);
        if (b) {
          acc += __popc(b);
          last = pos + 4u * j + ((31u - uint32_t(__clz(int(b)))) >> 3) + 1u;
          // the '\n' of this word at or after `from`
          const uint64_t base = pos + 4u * j;
          const uint32_t skip = from > base ? uint32_t(min(from - base, uint64_t(4))) : 0u;
          const uint32_t b2 = skip >= 4u ? 0u : b & ~((1u << (8u * skip)) - 1u);
          if (b2 && first == kNoPos) first = base + (uint32_t(__builtin_ctz(b2)) >> 3);
        }
      }
    }
  }
  acc = wave_sum64(acc);
  last = wave_max64(last);
  first = wave_min64(first);
  if ((threadIdx.x & 63) == 0) {
    part[0][threadIdx.x >> 6] = acc;
    part[1][threadIdx.x >> 6] = last;
    part[2][threadIdx.x >> 6] = first;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    partials[3 * blockIdx.x] = part[0][0] + part[0][1] + part[0][2] + part[0][3];
    partials[3 * blockIdx.x + 1] = max(max(part[1][0], part[1][1]), max(part[1][2], part[1][3]));
    partials[3 * blockIdx.x + 2] = min(min(part[2][0], part[2][1]), min(part[2][2], part[2][3]));
  }
}

// one workgroup folds the nblocks partials
__global__ __launch_bounds__(kThreads) void cut_finish_kernel(const unsigned long long* __restrict__ partials,
                                                              uint32_t nblocks, unsigned long long* __restrict__ cut) {
  __shared__ unsigned long long part[3][kThreads / 64];
  unsigned long long acc = 0, last = 0, first = kNoPos;
  for (uint32_t b = threadIdx.x; b < nblocks; b += kThreads) {
    acc += partials[3 * b];
    last = max(last, partials[3 * b + 1]);
    first = min(first, partials[3 * b + 2]);
  }
  acc = wave_sum64(acc);
  last = wave_max64(last);
  first = wave_min64(first);
  if ((threadIdx.x & 63) == 0) {
    part[0][threadIdx.x >> 6] = acc;
    part[1][threadIdx.x >> 6] = last;
    part[2][threadIdx.x >> 6] = first;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned long long f = min(min(part[2][0], part[2][1]), min(part[2][2], part[2][3]));
    cut[0] = max(max(part[1][0], part[1][1]), max(part[1][2], part[1][3]));
    cut[1] = part[0][0] + part[0][1] + part[0][2] + part[0][3];
    cut[2] = f == kNoPos ? 0ull : f + 1;
  }
}

// one thread per record
__global__ __launch_bounds__(kThreads) void rebase_append_kernel(const uint64_t* __restrict__ line_no,
                                                                 const uint64_t* __restrict__ start,
                                                                 const uint64_t* __restrict__ len, uint64_t nrec,
                                                                 uint64_t line_base, uint64_t byte_base,
                                                                 uint64_t* __restrict__ dst_line,
                                                                 uint64_t* __restrict__ dst_start,
                                                                 uint64_t* __restrict__ dst_len) {
  for (uint64_t r = uint64_t(blockIdx.x) * kThreads + threadIdx.x; r < nrec; r += uint64_t(gridDim.x) * kThreads) {
    dst_line[r] = line_no[r] + line_base;
    dst_start[r] = start[r] + byte_base;
    dst_len[r] = len[r];
  }
}

// One thread per record: its value_off entry, and the bytes of a short line.
// incl = the inclusive scan of len.
__global__ __launch_bounds__(kThreads) void gather_thread_kernel(GatherArgs a, const uint64_t* __restrict__ incl) {
  for (uint64_t r = uint64_t(blockIdx.x) * kThreads + threadIdx.x; r < a.nrec; r += uint64_t(gridDim.x) * kThreads) {
    const uint64_t end = incl[r], L = a.len[r];
    a.value_off[r + 1] = a.value_base + end;
    if (r + 1 == a.nrec) *a.total = end;
    if (L > kShortLine) continue;
    const uint8_t* __restrict__ src = a.data + a.start[r];
    uint8_t* __restrict__ dst = a.values + (end - L);
    for (uint64_t i = 0; i < L; ++i) dst[i] = src[i];
  }
}

// One wave per long line: the bytes up to the destination's first dword
// boundary and after its last one are stored byte by byte; a dword in between
// is one unaligned read of the window (two aligned dwords + v_alignbyte; the
// window buffer's allocation is padded past its last byte).
__global__ __launch_bounds__(kThreads) void gather_wave_kernel(GatherArgs a, const uint64_t* __restrict__ incl) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t nwaves = uint64_t(gridDim.x) * (kThreads / 64);
  for (uint64_t r = uint64_t(blockIdx.x) * (kThreads / 64) + (threadIdx.x >> 6); r < a.nrec; r += nwaves) {
    const uint64_t L = a.len[r];
    if (L <= kShortLine) continue;  // wave-uniform
    const uint64_t st = a.start[r], o = incl[r] - L;
    const uint64_t head = min(L, (4u - (o & 3u)) & 3u);
    const uint64_t words = (L - head) >> 2, tail0 = head + 4u * words;
    if (lane < head) a.values[o + lane] = a.data[st + lane];
    uint32_t* __restrict__ dw = reinterpret_cast<uint32_t*>(a.values + o + head);
    for (uint64_t k = lane; k < words; k += 64) {
      const uint64_t src = st + head + 4u * k;
      const uint32_t sh = uint32_t(src & 3u);
      const uint32_t* w = reinterpret_cast<const uint32_t*>(a.data + (src & ~uint64_t(3)));
      const uint32_t lo = w[0], hi = sh ? w[1] : 0u;
      dw[k] = __builtin_amdgcn_alignbyte(hi, lo, sh);
    }
    if (tail0 + lane < L) a.values[o + tail0 + lane] = a.data[st + tail0 + lane];
  }
}

inline size_t align256(size_t x) { return (x + 255) & ~size_t(255); }

int grid_for(uint64_t items, int num_cus) {
  const uint64_t blocks = (items + kThreads - 1) / kThreads;
  return int(std::max<uint64_t>(1, std::min<uint64_t>(blocks, uint64_t(std::max(num_cus, 1)) * 8)));
}

}  // namespace

hipError_t window_cut(const uint8_t* data, uint64_t n, uint64_t from, unsigned long long* partials,
                      unsigned long long* cut, int num_cus, hipStream_t s) {
  // 8 workgroups of 256 threads per CU keep every SIMD at 8 waves
  const uint64_t ntiles = std::max<uint64_t>(1, (n + kTile - 1) / kTile);
  const uint64_t want = std::min<uint64_t>(ntiles, std::min<uint64_t>(kCutBlocks, uint64_t(std::max(num_cus, 1)) * 8));
  const uint64_t tpb = (ntiles + want - 1) / want;
  const uint32_t grid = uint32_t((ntiles + tpb - 1) / tpb);
  hipLaunchKernelGGL(cut_kernel, dim3(grid), dim3(kThreads), 0, s, data, n, from, tpb, partials);
  hipLaunchKernelGGL(cut_finish_kernel, dim3(1), dim3(kThreads), 0, s, partials, grid, cut);
  return hipGetLastError();
}

hipError_t window_rebase_append(const uint64_t* line_no, const uint64_t* start, const uint64_t* len, uint64_t nrec,
                                uint64_t line_base, uint64_t byte_base, uint64_t* dst_line, uint64_t* dst_start,
                                uint64_t* dst_len, int num_cus, hipStream_t s) {
  if (nrec == 0) return hipSuccess;
  hipLaunchKernelGGL(rebase_append_kernel, dim3(grid_for(nrec, num_cus)), dim3(kThreads), 0, s, line_no, start, len,
                     nrec, line_base, byte_base, dst_line, dst_start, dst_len);
  return hipGetLastError();
}

hipError_t window_gather(const GatherArgs& a, void* scratch, size_t* scratch_bytes, int num_cus, hipStream_t s) {
  size_t tmp = 0;
  hipError_t e = hipcub::DeviceScan::InclusiveSum(nullptr, tmp, (const uint64_t*)nullptr, (uint64_t*)nullptr,
                                                  a.nrec, s);
  if (e != hipSuccess) return e;
  const size_t need = align256(size_t(a.nrec) * 8) + align256(tmp);
  if (!scratch || *scratch_bytes < need) {
    *scratch_bytes = need;
    return hipSuccess;
  }
  uint64_t* incl = static_cast<uint64_t*>(scratch);
  void* t = static_cast<uint8_t*>(scratch) + align256(size_t(a.nrec) * 8);
  if ((e = hipcub::DeviceScan::InclusiveSum(t, tmp, a.len, incl, a.nrec, s)) != hipSuccess) return e;
  hipLaunchKernelGGL(gather_thread_kernel, dim3(grid_for(a.nrec, num_cus)), dim3(kThreads), 0, s, a, incl);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  // one wave per record: 4 records per workgroup, at most 16384 workgroups
  const int wgrid = int(std::min<uint64_t>((a.nrec + 3) / 4, 16384));
  hipLaunchKernelGGL(gather_wave_kernel, dim3(wgrid), dim3(kThreads), 0, s, a, incl);
  return hipGetLastError();
}

}  // namespace dgrep
