// carry.hip — the exit state of a newline-free byte range under the blob's DFA
// (carry.h): one lane per chunk walks it from a few guessed entry states, one
// wave then follows the chain from the true one.
//
// Both kernels index the DFA by the blob's own state ids, entries u16 or u32.
// The byte-class table is held in LDS; the rows too while they fit kRowsLds
// bytes, else they are read through the caches. All LDS is dynamic, so its base
// stays 16-byte aligned. None of these kernels touches the scan kernels.
#include "carry.h"

#include <algorithm>

namespace dgrep {

namespace {

constexpr int kThreads = 256;            // 4 waves
constexpr uint64_t kRowsLds = kCarryRowsLds;
constexpr uint32_t G = kCarryGuesses;

struct ChunkArgs {
  const uint8_t* data;
  uint64_t m, chunk, nchunks;
  const void* trans;
  const uint8_t* cls;
  uint32_t nstates, nclasses, start;
  uint32_t seed[G];
  const uint32_t* state;  // the entry state, unless from_start
  uint32_t from_start, dual;
  uint32_t* guess;  // [nchunks][G]
  uint32_t* exit;   // [nchunks][G]
};

struct FixArgs {
  const uint8_t* data;
  uint64_t m, chunk, nchunks;
  const void* trans;
  const uint8_t* cls;
  const uint8_t* absorbing;
  uint32_t nclasses, start, start_m, nl_class;
  uint32_t* state;
  uint32_t from_start, dual;
  uint32_t* verdict;
  const uint32_t* guess;
  const uint32_t* exit;
  unsigned long long* counters;
};

// data[b : e) from the N states s[], b 16-byte aligned: 16-B loads, the bytes
// of a load in ascending order. cls and t may be LDS or global.
template <int N, typename T>
__device__ __forceinline__ void walk(const uint8_t* __restrict__ data, uint64_t b, uint64_t e,
                                     const uint8_t* cls, const T* t, uint32_t K, uint32_t (&s)[N]) {
  for (uint64_t pos = b; pos < e; pos += 16) {
    const uint4 v = *reinterpret_cast<const uint4*>(data + pos);
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    if (pos + 16 <= e) {
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const uint32_t c = cls[(w[j >> 2] >> (8 * (j & 3))) & 255u];
#pragma unroll
        for (int g = 0; g < N; ++g) s[g] = t[size_t(s[g]) * K + c];
      }
    } else {
      const int nb = int(e - pos);  // the range's last, partial load: bytes at or past e are ignored
      for (int j = 0; j < nb; ++j) {
        const uint32_t c = cls[(w[j >> 2] >> (8 * (j & 3))) & 255u];
#pragma unroll
        for (int g = 0; g < N; ++g) s[g] = t[size_t(s[g]) * K + c];
      }
    }
  }
}

// One lane per chunk: its guesses and, from each, its exit.
template <typename T, bool kLds>
__global__ __launch_bounds__(kThreads) void carry_chunk_kernel(ChunkArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  uint8_t* cls = smem;  // [256]
  T* rows = reinterpret_cast<T*>(smem + 256);
  const T* gt = static_cast<const T*>(a.trans);
  cls[threadIdx.x] = a.cls[threadIdx.x];
  if (kLds) {
    const uint32_t ne = a.nstates * a.nclasses;
    for (uint32_t i = threadIdx.x; i < ne; i += kThreads) rows[i] = gt[i];
  }
  __syncthreads();
  const T* t = kLds ? rows : gt;
  const uint32_t K = a.nclasses;
  const uint64_t ch = uint64_t(blockIdx.x) * kThreads + threadIdx.x;
  if (ch >= a.nchunks) return;
  const uint64_t b = ch * a.chunk, e = min(a.m, b + a.chunk);
  uint32_t s[G];
  if (ch == 0) {
    const uint32_t entry = a.from_start ? a.start : *a.state;
#pragma unroll
    for (uint32_t g = 0; g < G; ++g) s[g] = (a.dual && (g & 1u)) ? a.start : entry;
  } else {
    // chunk >= kCarryLookback, so the lookback never reaches before the range
#pragma unroll
    for (uint32_t g = 0; g < G; ++g) s[g] = a.seed[g];
    walk<int(G)>(a.data, b - kCarryLookback, b, cls, t, K, s);
  }
  *reinterpret_cast<uint4*>(a.guess + ch * G) = make_uint4(s[0], s[1], s[2], s[3]);
  if (s[0] == s[1] && s[1] == s[2] && s[2] == s[3]) {
    // the seeds met: one walk serves all four
    uint32_t one[1] = {s[0]};
    walk<1>(a.data, b, e, cls, t, K, one);
    s[0] = s[1] = s[2] = s[3] = one[0];
  } else {
    walk<int(G)>(a.data, b, e, cls, t, K, s);
  }
  *reinterpret_cast<uint4*>(a.exit + ch * G) = make_uint4(s[0], s[1], s[2], s[3]);
}

// One wave. Lane l holds the pairs of chunks base + 64 j + l, j < kFixPer, in
// registers (two 16-byte loads per chunk, a wave's loads contiguous), the next
// batch's are loaded while this one is followed. The chain itself is
// wave-uniform: chunk i's pairs come out of lane i with v_readlane and the
// state stays scalar, so a step costs a few scalar instructions instead of two
// LDS round trips (one thread over LDS: 150 ns a chunk, 155 ms for the 2^20
// chunks of a 1 GiB line). `second` follows the same chain from `start`
// (dual). A state that is not among a chunk's guesses is tested for absorbing
// first -- a dependent global load, so only there: the seeds are never
// absorbing, so an absorbing state misses at once unless the lookback itself
// reached it -- and is then left alone for the rest of the range; else every
// lane walks the chunk again from it (the same addresses in all lanes).
constexpr int kFixLanes = 64, kFixPer = 4;

__device__ __forceinline__ uint32_t lane_get(uint32_t v, uint32_t i) {
  return uint32_t(__builtin_amdgcn_readlane(int(v), int(i)));
}

template <typename T>
__global__ __launch_bounds__(kFixLanes) void carry_fix_kernel(FixArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  uint8_t* cls = smem;  // [256]
  const T* t = static_cast<const T*>(a.trans);
  const uint32_t K = a.nclasses, lane = threadIdx.x;
  for (uint32_t i = lane; i < 256; i += kFixLanes) cls[i] = a.cls[i];
  __syncthreads();
  uint32_t st = a.from_start ? a.start : *a.state, st2 = a.start;
  bool still = false, still2 = !a.dual;  // the state is absorbing (or there is no second chain)
  unsigned long long misses = 0;
  uint4 g[kFixPer], x[kFixPer], gn[kFixPer], xn[kFixPer];
  auto load = [&](uint64_t base, uint4(&gg)[kFixPer], uint4(&xx)[kFixPer]) {
#pragma unroll
    for (int j = 0; j < kFixPer; ++j) {
      const uint64_t ch = base + uint64_t(j) * kFixLanes + lane;
      const bool in = ch < a.nchunks;
      gg[j] = in ? *reinterpret_cast<const uint4*>(a.guess + ch * G) : make_uint4(0u, 0u, 0u, 0u);
      xx[j] = in ? *reinterpret_cast<const uint4*>(a.exit + ch * G) : make_uint4(0u, 0u, 0u, 0u);
    }
  };
  // the state after chunk ch, entered in state s that is not among its guesses
  auto again = [&](uint32_t s, uint64_t ch, bool* absorbing) -> uint32_t {
    if (a.absorbing[s]) {
      *absorbing = true;
      return s;
    }
    const uint64_t b = ch * a.chunk, e = min(a.m, b + a.chunk);
    uint32_t one[1] = {s};
    walk<1>(a.data, b, e, cls, t, K, one);
    return uint32_t(__builtin_amdgcn_readfirstlane(int(one[0])));
  };
  constexpr uint64_t kBatch = uint64_t(kFixLanes) * kFixPer;
  load(0, g, x);
  for (uint64_t base = 0; base < a.nchunks; base += kBatch) {
    // once per batch, so that a state the lookbacks reach too (it never misses) still ends the chain
    if (!still && a.absorbing[st]) still = true;
    if (!still2 && a.absorbing[st2]) still2 = true;
    if (still && still2) break;
    if (base + kBatch < a.nchunks) load(base + kBatch, gn, xn);
#pragma unroll
    for (int j = 0; j < kFixPer; ++j) {
      const uint64_t first = base + uint64_t(j) * kFixLanes;
      const uint32_t cnt = first < a.nchunks ? uint32_t(min(uint64_t(kFixLanes), a.nchunks - first)) : 0u;
      for (uint32_t i = 0; i < cnt; ++i) {
        const uint32_t g0 = lane_get(g[j].x, i), g1 = lane_get(g[j].y, i), g2 = lane_get(g[j].z, i),
                       g3 = lane_get(g[j].w, i);
        const uint32_t x0 = lane_get(x[j].x, i), x1 = lane_get(x[j].y, i), x2 = lane_get(x[j].z, i),
                       x3 = lane_get(x[j].w, i);
        if (!still) {
          if (st == g0) st = x0;
          else if (st == g1) st = x1;
          else if (st == g2) st = x2;
          else if (st == g3) st = x3;
          else {
            st = again(st, first + i, &still);
            if (!still) ++misses;
          }
        }
        if (!still2) {
          if (st2 == g0) st2 = x0;
          else if (st2 == g1) st2 = x1;
          else if (st2 == g2) st2 = x2;
          else if (st2 == g3) st2 = x3;
          else st2 = again(st2, first + i, &still2);
        }
      }
    }
#pragma unroll
    for (int j = 0; j < kFixPer; ++j) {
      g[j] = gn[j];
      x[j] = xn[j];
    }
  }
  if (lane == 0) {
    *a.state = st;
    if (a.verdict) {
      a.verdict[0] = uint32_t(t[size_t(st) * K + a.nl_class]) == a.start_m ? 1u : 0u;
      a.verdict[1] = a.dual && uint32_t(t[size_t(st2) * K + a.nl_class]) == a.start_m ? 1u : 0u;
    }
    a.counters[0] += a.nchunks;
    a.counters[1] += misses;
  }
}

__global__ void carry_put_record_kernel(uint64_t* __restrict__ dst_line, uint64_t* __restrict__ dst_start,
                                        uint64_t* __restrict__ dst_len, uint64_t line_no, uint64_t start,
                                        uint64_t len) {
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    dst_line[0] = line_no;
    dst_start[0] = start;
    dst_len[0] = len;
  }
}

template <typename T>
hipError_t launch(const CarryTable& t, const CarryWalk& w, const CarryPlan& plan, hipStream_t s) {
  uint32_t* guess = w.pairs;
  uint32_t* exit = w.pairs + plan.nchunks * G;
  if (plan.nchunks) {
    ChunkArgs a;
    a.data = w.data;
    a.m = w.m;
    a.chunk = plan.chunk;
    a.nchunks = plan.nchunks;
    a.trans = t.trans;
    a.cls = t.cls;
    a.nstates = t.nstates;
    a.nclasses = t.nclasses;
    a.start = t.start;
    for (uint32_t g = 0; g < G; ++g) a.seed[g] = t.seed[g];
    a.state = w.state;
    a.from_start = w.from_start ? 1u : 0u;
    a.dual = w.dual ? 1u : 0u;
    a.guess = guess;
    a.exit = exit;
    const uint64_t rows_bytes = uint64_t(t.nstates) * t.nclasses * sizeof(T);
    const uint32_t grid = uint32_t((plan.nchunks + kThreads - 1) / kThreads);
    if (rows_bytes <= kRowsLds)
      hipLaunchKernelGGL((carry_chunk_kernel<T, true>), dim3(grid), dim3(kThreads),
                         256 + ((size_t(rows_bytes) + 15) & ~size_t(15)), s, a);
    else
      hipLaunchKernelGGL((carry_chunk_kernel<T, false>), dim3(grid), dim3(kThreads), 256, s, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  FixArgs f;
  f.data = w.data;
  f.m = w.m;
  f.chunk = plan.chunk;
  f.nchunks = plan.nchunks;
  f.trans = t.trans;
  f.cls = t.cls;
  f.absorbing = t.absorbing;
  f.nclasses = t.nclasses;
  f.start = t.start;
  f.start_m = t.start_m;
  f.nl_class = t.nl_class;
  f.state = w.state;
  f.from_start = w.from_start ? 1u : 0u;
  f.dual = w.dual ? 1u : 0u;
  f.verdict = w.verdict;
  f.guess = guess;
  f.exit = exit;
  f.counters = w.counters;
  hipLaunchKernelGGL((carry_fix_kernel<T>), dim3(1), dim3(kFixLanes), 256, s, f);
  return hipGetLastError();
}

}  // namespace

hipError_t carry_walk(const CarryTable& t, const CarryWalk& w, const CarryPlan& plan, hipStream_t s) {
  if (!t.trans || !t.cls || !t.absorbing || !w.state || !w.counters || (w.m && !w.data) ||
      (plan.nchunks && !w.pairs) || plan.chunk < kCarryLookback || plan.chunk % 16 ||
      plan.nchunks != w.m / plan.chunk + (w.m % plan.chunk ? 1 : 0) ||
      plan.nchunks > (uint64_t(1) << 31))
    return hipErrorInvalidValue;
  return t.u32 ? launch<uint32_t>(t, w, plan, s) : launch<uint16_t>(t, w, plan, s);
}

hipError_t carry_put_record(uint64_t* dst_line, uint64_t* dst_start, uint64_t* dst_len, uint64_t line_no,
                            uint64_t start, uint64_t len, hipStream_t s) {
  hipLaunchKernelGGL(carry_put_record_kernel, dim3(1), dim3(64), 0, s, dst_line, dst_start, dst_len, line_no, start,
                     len);
  return hipGetLastError();
}

}  // namespace dgrep
