// job_arena.hip — append one flush's or one window's encoded bytes and cell
// boundaries to the job's device arena (job_arena.h).
//
// A plain streaming copy whose destination has any byte alignment. The source
// is 16-byte aligned, so with h = the bytes up to the destination's first
// 16-byte boundary, destination vector j holds source bytes [h + 16 j, h + 16 j
// + 16): source vectors j and j + 1 shifted right by h bytes. Each lane loads
// the two vectors with 16-byte loads (its neighbour's second is its own first:
// the second load hits L1/L2), funnel-shifts them with v_alignbyte_b32 and
// stores one aligned 16-byte vector. The word part of the shift (h / 4) selects
// among registers, so it is a template argument picked by a kernel-uniform
// switch: no runtime-indexed array, no scratch. Head (< 16 bytes) and tail
// (< 16 bytes) go bytewise. With h > 0, vector j + 1 begins at source byte
// 16 j + 16 < h + 16 j + 16 <= total, so it lies within `total` rounded up to
// 16; with h == 0 it is not loaded.
#include "job_arena.h"

#include <hipcub/hipcub.hpp>

namespace dgrep {

namespace {

constexpr int kArenaThreads = 256;
constexpr int kArenaBlocksPerCu = 8;

// words WS .. WS + 4 of lo:hi, shifted right by `bs` bytes (bs in 0..3)
template <int WS>
__device__ __forceinline__ uint4 funnel(const uint4 lo, const uint4 hi, uint32_t bs) {
  const uint32_t w[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
  uint4 o;
  o.x = __builtin_amdgcn_alignbyte(w[WS + 1], w[WS + 0], bs);
  o.y = __builtin_amdgcn_alignbyte(w[WS + 2], w[WS + 1], bs);
  o.z = __builtin_amdgcn_alignbyte(w[WS + 3], w[WS + 2], bs);
  o.w = __builtin_amdgcn_alignbyte(w[WS + 4], w[WS + 3], bs);
  return o;
}

template <int WS>
__device__ __forceinline__ void copy_shifted(const uint4* __restrict__ sv, uint4* __restrict__ dv, uint64_t vecs,
                                             uint32_t bs, uint64_t tid, uint64_t nthr) {
#pragma unroll 2
  for (uint64_t j = tid; j < vecs; j += nthr) dv[j] = funnel<WS>(sv[j], sv[j + 1], bs);
}

__global__ __launch_bounds__(kArenaThreads) void arena_append_kernel(ArenaAppendArgs a) {
  const uint64_t tid = uint64_t(blockIdx.x) * kArenaThreads + threadIdx.x;
  const uint64_t nthr = uint64_t(gridDim.x) * kArenaThreads;
  // (b) the rebased cell boundaries
  if (!a.running_max) {
    for (uint64_t i = tid; i < a.nend; i += nthr) a.seg[i] = a.used + a.src_end[i];
  } else if (blockIdx.x == 0) {
    // A window's partition ends: an empty partition's is 0, the others ascend, so
    // cell i ends at the running maximum. One workgroup scans them in steps of
    // its size with the maximum so far carried along; the others copy meanwhile.
    using Scan = hipcub::BlockScan<uint64_t, kArenaThreads>;
    __shared__ typename Scan::TempStorage tmp;
    uint64_t carry = 0;
    for (uint64_t base = 0; base < a.nend; base += kArenaThreads) {
      const uint64_t i = base + threadIdx.x;
      uint64_t v = i < a.nend ? a.src_end[i] : 0, step_max = 0;
      Scan(tmp).InclusiveScan(v, v, hipcub::Max(), step_max);
      if (v < carry) v = carry;
      if (i < a.nend) a.seg[i] = a.used + v;
      if (carry < step_max) carry = step_max;
      __syncthreads();  // tmp is reused by the next step
    }
  }
  // (a) the bytes
  uint8_t* __restrict__ dst = a.arena + a.used;
  const uint8_t* __restrict__ src = a.src;
  uint64_t head = (16 - (a.used & 15)) & 15;
  if (head > a.total) head = a.total;
  const uint64_t vecs = (a.total - head) / 16;
  const uint64_t tail_at = head + 16 * vecs;
  if (tid < head) dst[tid] = src[tid];
  if (tid < a.total - tail_at) dst[tail_at + tid] = src[tail_at + tid];
  const uint4* sv = reinterpret_cast<const uint4*>(src);
  uint4* dv = reinterpret_cast<uint4*>(dst + head);
  if (head == 0) {
#pragma unroll 2
    for (uint64_t j = tid; j < vecs; j += nthr) dv[j] = sv[j];
    return;
  }
  const uint32_t bs = uint32_t(head) & 3;
  switch (uint32_t(head) >> 2) {  // the same in every lane of the launch
    case 0: copy_shifted<0>(sv, dv, vecs, bs, tid, nthr); break;
    case 1: copy_shifted<1>(sv, dv, vecs, bs, tid, nthr); break;
    case 2: copy_shifted<2>(sv, dv, vecs, bs, tid, nthr); break;
    default: copy_shifted<3>(sv, dv, vecs, bs, tid, nthr); break;
  }
}

}  // namespace

hipError_t arena_append(const ArenaAppendArgs& a, int num_cus, hipStream_t s) {
  if (a.total == 0 && a.nend == 0) return hipSuccess;
  const uint64_t work = (a.total / 16 > a.nend ? a.total / 16 : a.nend) + 32;  // (+ the head's and the tail's lanes)
  uint64_t blocks = (work + kArenaThreads - 1) / kArenaThreads;
  const uint64_t cap = uint64_t(num_cus > 0 ? num_cus : 1) * kArenaBlocksPerCu;
  if (blocks > cap) blocks = cap;
  hipLaunchKernelGGL(arena_append_kernel, dim3(uint32_t(blocks)), dim3(kArenaThreads), 0, s, a);
  return hipGetLastError();
}

}  // namespace dgrep
