// reduce_batch.hip — all reduce tasks of a job in one pass over one buffer.
//
// Reference (map_reduce/worker.go): reduce task r reads mr-0-<r>, mr-1-<r>, ...
// (readReduceInput, 44-68), keeps one value per distinct key
// (reduceDistinctKeys, 22-42, with the grep plugin's Reduce = values[0],
// application/grep.go:38-40) and writes "key value\n" lines to mr-out-<r>
// (161-165). reduce.hip does that for one r from the host's bytes; here the
// bytes of every r sit in one device buffer, cut into segments (reduce_batch.h),
// and every mr-out-<r> comes out of one launch train:
//   newline positions over the whole buffer (the two SWAR passes of reduce.hip);
//   measure: one thread per line finds the line's segment (the last segment
//     that starts at or before the line's '\n': empty segments are skipped by
//     construction) and so its partition, then decodes as reduce.hip does;
//   placement: a stable radix sort of the line ids by partition, over
//     ceil(log2 nparts) bits, gives the partition-major, input-ordered line
//     list; the partitions' first lines in it by lower bound;
//   malformed input: the lowest (partition, line) of the lines outside the
//     accepted form and of the segments that do not end in '\n';
//   grouping: the 64-bit radix sort of (key hash, line) of reduce.hip; inside
//     an equal-hash run a line is compared only with lines of its own
//     partition, so the same key in two partitions is kept in both;
//   an exclusive sum of the kept lengths in placed order, the partitions'
//     offsets read from it, and the writer: one wave per 64 placed lines.
// The accepted line language is reduce.hip's (reduce_common.h).
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include "reduce_batch.h"
#include "reduce_common.h"

namespace dgrep {
namespace {

constexpr uint8_t kFlagPlain = 1, kFlagBad = 2;

// Line j = (a, e): e its '\n', a the byte after the previous '\n', or its
// segment's first byte where the previous segment left a line unfinished (that
// segment is reported by bad_kernel; this line is judged as the reference
// would judge the first line of the segment's file).
__global__ __launch_bounds__(kRT) void measure_batch_kernel(const uint8_t* s, const uint64_t* nl, uint64_t nlines,
                                                            const uint64_t* seg_off, uint64_t nseg, uint32_t nparts,
                                                            uint64_t* klen, uint64_t* vlen, uint64_t* kh,
                                                            uint32_t* idx, uint8_t* flags, uint32_t* part) {
  for (uint64_t j = uint64_t(blockIdx.x) * kRT + threadIdx.x; j < nlines; j += uint64_t(gridDim.x) * kRT) {
    const uint64_t e = nl[j];
    uint64_t lo = 0, hi = nseg;  // seg_off[lo] <= e < seg_off[hi]
    while (hi - lo > 1) {
      const uint64_t mid = lo + ((hi - lo) >> 1);
      if (seg_off[mid] <= e) lo = mid;
      else hi = mid;
    }
    const uint64_t a = max(j ? nl[j - 1] + 1 : 0, seg_off[lo]);
    bool pl;
    uint8_t f = 0;
    if (!parse_line<false>(s, a, e, nullptr, &klen[j], &vlen[j], &kh[j], &pl)) {
      f = kFlagBad;
      klen[j] = vlen[j] = 0;
      kh[j] = 0;
    } else if (pl) {
      f = kFlagPlain;
    }
    flags[j] = f;
    part[j] = uint32_t(lo % nparts);
    idx[j] = uint32_t(j);
  }
}

// first q in [lo, hi) with v[q] >= x (hi if none)
__device__ __forceinline__ uint64_t lower_bound_u32(const uint32_t* v, uint64_t lo, uint64_t hi, uint32_t x) {
  while (lo < hi) {
    const uint64_t mid = lo + ((hi - lo) >> 1);
    if (v[mid] < x) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// line_start[p] (nparts + 1): partition p's first line in placed order;
// lines_in[p]: its lines.
__global__ __launch_bounds__(kRT) void line_start_kernel(const uint32_t* part_sorted, uint64_t nlines, uint32_t nparts,
                                                         uint64_t* line_start, uint64_t* lines_in) {
  const uint32_t p = blockIdx.x * kRT + threadIdx.x;
  if (p > nparts) return;
  const uint64_t b = lower_bound_u32(part_sorted, 0, nlines, p);
  line_start[p] = b;
  if (p < nparts) lines_in[p] = lower_bound_u32(part_sorted, b, nlines, p + 1) - b;
}

// *bad = the lowest (partition, line in the partition's input) that is
// malformed (reduce_batch.h, d_info[1]): a flagged line, or the unfinished last
// line of a non-empty segment that does not end in '\n' -- the line after the
// partition's lines that end before the segment's end.
__global__ __launch_bounds__(kRT) void bad_kernel(const uint8_t* s, const uint64_t* nl, uint64_t nlines,
                                                  const uint32_t* order, const uint32_t* part_sorted,
                                                  const uint8_t* flags, const uint64_t* line_start,
                                                  const uint64_t* seg_off, uint64_t nseg, uint32_t nparts,
                                                  unsigned long long* bad) {
  const uint64_t t0 = uint64_t(blockIdx.x) * kRT + threadIdx.x, step = uint64_t(gridDim.x) * kRT;
  for (uint64_t q = t0; q < nlines; q += step) {
    if (!(flags[order[q]] & kFlagBad)) continue;
    const uint64_t p = part_sorted[q];
    atomicMin(bad, (unsigned long long)((p << 34) | ((q - line_start[p]) << 1) | 1u));
  }
  for (uint64_t g = t0; g < nseg; g += step) {
    const uint64_t b = seg_off[g], e = seg_off[g + 1];
    if (e == b || s[e - 1] == '\n') continue;
    const uint64_t p = g % nparts, first = line_start[p];
    uint64_t lo = first, hi = line_start[p + 1];
    while (lo < hi) {
      const uint64_t mid = lo + ((hi - lo) >> 1);
      if (nl[order[mid]] < e) lo = mid + 1;
      else hi = mid;
    }
    atomicMin(bad, (unsigned long long)((p << 34) | ((lo - first) << 1)));
  }
}

// dedupe_kernel of reduce.hip with the partition rule: keep[line] = 1 unless an
// earlier line OF THE SAME PARTITION in the same equal-hash run has the
// identical decoded key. The sort is by (hash, line), and buffer line order
// restricted to one partition is that partition's input order. With a
// malformed line anywhere nothing is kept: the call fails. (No line then
// needs its start: every segment ends in '\n', so a line starts after the
// previous '\n'.)
__global__ __launch_bounds__(kRT) void dedupe_batch_kernel(const uint8_t* s, const uint64_t* nl,
                                                           const uint64_t* h_sorted, const uint32_t* idx_sorted,
                                                           uint64_t nlines, const uint64_t* klen,
                                                           const uint64_t* vlen, const uint32_t* part,
                                                           uint64_t* out_len, const unsigned long long* bad) {
  const bool any_bad = *bad != ~0ull;
  for (uint64_t q = uint64_t(blockIdx.x) * kRT + threadIdx.x; q < nlines; q += uint64_t(gridDim.x) * kRT) {
    const uint32_t j = idx_sorted[q];
    bool keep = !any_bad;
    for (uint64_t p = q; keep && p-- > 0 && h_sorted[p] == h_sorted[q];) {
      const uint32_t k = idx_sorted[p];
      if (part[k] != part[j]) continue;  // the same key in another partition is another key
      if (klen[k] != klen[j]) continue;
      const uint64_t aj = j ? nl[j - 1] + 1 : 0, ak = k ? nl[k - 1] + 1 : 0;
      bool same = true;
      for (uint64_t t = 8;; ++t) {
        const uint8_t x = s[aj + t], y = s[ak + t];
        if (x != y) { same = false; break; }
        if (x == '"') break;  // the closing quote (escaped ones are skipped below)
        if (x == '\\') {
          ++t;
          if (s[aj + t] != s[ak + t]) { same = false; break; }
        }
      }
      if (!same) {  // another spelling of the same key? (equal hash and length: almost surely)
        KeyBytes cj(s, aj + 8, nl[j]), ck(s, ak + 8, nl[k]);
        same = true;
        for (uint64_t t = 0; t < klen[j]; ++t)
          if (cj.next() != ck.next()) { same = false; break; }
      }
      if (same) keep = false;
    }
    out_len[j] = keep ? klen[j] + 1 + vlen[j] + 1 : 0;
  }
}

// the kept lengths in placed order
__global__ __launch_bounds__(kRT) void place_len_kernel(const uint64_t* out_len, const uint32_t* order,
                                                        uint64_t nlines, uint64_t* plen) {
  for (uint64_t q = uint64_t(blockIdx.x) * kRT + threadIdx.x; q < nlines; q += uint64_t(gridDim.x) * kRT)
    plen[q] = out_len[order[q]];
}

// part_off[p] = the position of partition p's first placed line (the total for
// the partitions after the last line); *total.
__global__ __launch_bounds__(kRT) void part_off_kernel(const uint64_t* ppos, const uint64_t* plen, uint64_t nlines,
                                                       const uint64_t* line_start, uint32_t nparts,
                                                       uint64_t* part_off, uint64_t* total) {
  const uint32_t p = blockIdx.x * kRT + threadIdx.x;
  if (p > nparts) return;
  const uint64_t all = ppos[nlines - 1] + plen[nlines - 1];
  const uint64_t q = line_start[p];
  part_off[p] = q < nlines ? ppos[q] : all;
  if (p == nparts) *total = all;
}

// write_kernel of reduce.hip with the line read through the placed order: one
// WAVE per 64 placed lines (which may span partitions and segments); lane l
// fetches placed line q0 + l's extents, then the wave walks the 64 lines.
__global__ __launch_bounds__(kRT) void write_batch_kernel(const uint8_t* s, uint64_t n, const uint64_t* nl,
                                                          uint64_t nlines, const uint32_t* order,
                                                          const uint64_t* klen, const uint64_t* vlen,
                                                          const uint8_t* flags, const uint64_t* plen,
                                                          const uint64_t* ppos, uint8_t* out, uint64_t out_cap) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t nwaves = uint64_t(gridDim.x) * (kRT / 64);
  for (uint64_t q0 = (uint64_t(blockIdx.x) * (kRT / 64) + (threadIdx.x >> 6)) * 64u; q0 < nlines; q0 += nwaves * 64u) {
    const uint64_t qm = q0 + lane;
    uint64_t a = 0, e = 0, kl = 0, vl = 0, ol = 0, P = 0;
    int pl = 0;
    if (qm < nlines) {
      ol = plen[qm];
      P = ppos[qm];
      if (ol) {
        const uint32_t jm = order[qm];
        a = jm ? nl[jm - 1] + 1 : 0;
        e = nl[jm];
        kl = klen[jm];
        vl = vlen[jm];
        pl = flags[jm] & kFlagPlain;
      }
    }
    const uint32_t cnt = uint32_t(min(uint64_t(64), nlines - q0));
    for (uint32_t r = 0; r < cnt; ++r) {
      const uint64_t olr = __shfl(ol, int(r), 64), Pr = __shfl(P, int(r), 64);
      if (!olr || Pr + olr > out_cap) continue;
      const uint64_t ar = __shfl(a, int(r), 64);
      const uint64_t klr = __shfl(kl, int(r), 64), vlr = __shfl(vl, int(r), 64);
      if (!__shfl(pl, int(r), 64)) {  // escapes or coerced bytes inside: decoded by the line's lane
        if (lane == r) {
          uint64_t x, y, h;
          bool f;
          parse_line<true>(s, a, e, out + P, &x, &y, &h, &f);
        }
        continue;
      }
      write_plain_dwords(s, n, out, lane, Pr, olr, ar, klr, vlr);
    }
  }
}

inline int sort_bits(uint32_t nparts) {
  int b = 0;
  while ((uint64_t(1) << b) < nparts) ++b;
  return b;
}
}  // namespace

hipError_t reduce_batch(const ReduceBatchArgs& a, void* scratch, size_t* scratch_bytes, uint8_t* out,
                        uint64_t out_cap, uint64_t* d_part_off, uint64_t* d_lines_in, uint64_t* d_info,
                        hipStream_t s) {
  const uint64_t nlines = a.nlines, n = a.n;
  const uint64_t L = std::max<uint64_t>(nlines, 1);
  const uint64_t nblk = std::max<uint64_t>((n + kSeg - 1) / kSeg, 1);
  const int pbits = sort_bits(a.nparts);
  size_t sel_tmp = 0, sort_tmp = 0, psort_tmp = 0, scan_tmp = 0;
  hipError_t e = hipcub::DeviceScan::ExclusiveSum(nullptr, sel_tmp, (uint64_t*)nullptr, (uint64_t*)nullptr, nblk, s);
  if (e != hipSuccess) return e;
  if ((e = hipcub::DeviceRadixSort::SortPairs(nullptr, sort_tmp, (uint64_t*)nullptr, (uint64_t*)nullptr,
                                              (uint32_t*)nullptr, (uint32_t*)nullptr, L, 0, 64, s)) != hipSuccess)
    return e;
  if ((e = hipcub::DeviceRadixSort::SortPairs(nullptr, psort_tmp, (uint32_t*)nullptr, (uint32_t*)nullptr,
                                              (uint32_t*)nullptr, (uint32_t*)nullptr, L, 0, std::max(pbits, 1), s)) !=
      hipSuccess)
    return e;
  if ((e = hipcub::DeviceScan::ExclusiveSum(nullptr, scan_tmp, (uint64_t*)nullptr, (uint64_t*)nullptr, L, s)) !=
      hipSuccess)
    return e;
  const size_t tmp = std::max({sel_tmp, sort_tmp, psort_tmp, scan_tmp});
  const size_t need = a256(L * 8) * 8 + a256(L * 4) * 5 + a256(L) + a256(tmp) + 2 * a256(nblk * 8) +
                      a256((uint64_t(a.nparts) + 1) * 8);
  if (!scratch || *scratch_bytes < need) {
    *scratch_bytes = need;
    return hipSuccess;
  }
  uint8_t* p = static_cast<uint8_t*>(scratch);
  auto take = [&](size_t b) {
    uint8_t* q = p;
    p += a256(b);
    return q;
  };
  uint64_t* nl = reinterpret_cast<uint64_t*>(take(L * 8));
  uint64_t* klen = reinterpret_cast<uint64_t*>(take(L * 8));
  uint64_t* vlen = reinterpret_cast<uint64_t*>(take(L * 8));
  uint64_t* kh = reinterpret_cast<uint64_t*>(take(L * 8));
  uint64_t* kh_sorted = reinterpret_cast<uint64_t*>(take(L * 8));
  uint64_t* out_len = reinterpret_cast<uint64_t*>(take(L * 8));
  uint64_t* plen = reinterpret_cast<uint64_t*>(take(L * 8));
  uint64_t* ppos = reinterpret_cast<uint64_t*>(take(L * 8));
  uint32_t* idx = reinterpret_cast<uint32_t*>(take(L * 4));
  uint32_t* idx_sorted = reinterpret_cast<uint32_t*>(take(L * 4));
  uint32_t* part = reinterpret_cast<uint32_t*>(take(L * 4));
  uint32_t* part_sorted = reinterpret_cast<uint32_t*>(take(L * 4));
  uint32_t* order = reinterpret_cast<uint32_t*>(take(L * 4));
  uint8_t* flags = take(L);
  void* t = take(tmp);
  uint64_t* blk_cnt = reinterpret_cast<uint64_t*>(take(nblk * 8));
  uint64_t* blk_off = reinterpret_cast<uint64_t*>(take(nblk * 8));
  uint64_t* line_start = reinterpret_cast<uint64_t*>(take((uint64_t(a.nparts) + 1) * 8));
  unsigned long long* bad = reinterpret_cast<unsigned long long*>(d_info + 1);
  const int pgrid = int((a.nparts + 1 + kRT - 1) / kRT);

  if ((e = hipMemsetAsync(d_info, 0, 8, s)) != hipSuccess) return e;
  if ((e = hipMemsetAsync(d_info + 1, 0xff, 8, s)) != hipSuccess) return e;
  if ((e = hipMemsetAsync(d_info + 2, 0, 8, s)) != hipSuccess) return e;
  if (n == 0 || nlines == 0) {
    if ((e = hipMemsetAsync(d_part_off, 0, (uint64_t(a.nparts) + 1) * 8, s)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(d_lines_in, 0, uint64_t(a.nparts) * 8, s)) != hipSuccess) return e;
    if (n == 0) return hipSuccess;
    // bytes without a '\n': the first non-empty segment's unfinished line
    if ((e = hipMemsetAsync(line_start, 0, (uint64_t(a.nparts) + 1) * 8, s)) != hipSuccess) return e;
    hipLaunchKernelGGL(bad_kernel, dim3(grid_of(a.nseg)), dim3(kRT), 0, s, a.data, nl, uint64_t(0), order,
                       part_sorted, flags, line_start, a.seg_off, a.nseg, a.nparts, bad);
    return hipGetLastError();
  }
  size_t tb = tmp;
  hipLaunchKernelGGL(nl_count_kernel, dim3(nblk), dim3(kRT), 0, s, a.data, n, blk_cnt);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if ((e = hipcub::DeviceScan::ExclusiveSum(t, tb, blk_cnt, blk_off, nblk, s)) != hipSuccess) return e;
  hipLaunchKernelGGL(nl_write_kernel, dim3(nblk), dim3(kRT), 0, s, a.data, n, blk_off, nl);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipLaunchKernelGGL(nl_total_kernel, dim3(1), dim3(1), 0, s, blk_off, blk_cnt, nblk, d_info);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipLaunchKernelGGL(measure_batch_kernel, dim3(grid_of(nlines)), dim3(kRT), 0, s, a.data, nl, nlines, a.seg_off,
                     a.nseg, a.nparts, klen, vlen, kh, idx, flags, part);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if (pbits == 0) {  // one partition: the placed order is the line order
    if ((e = hipMemcpyAsync(order, idx, nlines * 4, hipMemcpyDeviceToDevice, s)) != hipSuccess) return e;
    if ((e = hipMemcpyAsync(part_sorted, part, nlines * 4, hipMemcpyDeviceToDevice, s)) != hipSuccess) return e;
  } else {
    tb = tmp;
    if ((e = hipcub::DeviceRadixSort::SortPairs(t, tb, part, part_sorted, idx, order, nlines, 0, pbits, s)) !=
        hipSuccess)
      return e;
  }
  hipLaunchKernelGGL(line_start_kernel, dim3(pgrid), dim3(kRT), 0, s, part_sorted, nlines, a.nparts, line_start,
                     d_lines_in);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipLaunchKernelGGL(bad_kernel, dim3(grid_of(std::max(nlines, a.nseg))), dim3(kRT), 0, s, a.data, nl, nlines, order,
                     part_sorted, flags, line_start, a.seg_off, a.nseg, a.nparts, bad);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  tb = tmp;
  if ((e = hipcub::DeviceRadixSort::SortPairs(t, tb, kh, kh_sorted, idx, idx_sorted, nlines, 0, 64, s)) != hipSuccess)
    return e;
  hipLaunchKernelGGL(dedupe_batch_kernel, dim3(grid_of(nlines)), dim3(kRT), 0, s, a.data, nl, kh_sorted, idx_sorted,
                     nlines, klen, vlen, part, out_len, bad);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipLaunchKernelGGL(place_len_kernel, dim3(grid_of(nlines)), dim3(kRT), 0, s, out_len, order, nlines, plen);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  tb = tmp;
  if ((e = hipcub::DeviceScan::ExclusiveSum(t, tb, plen, ppos, nlines, s)) != hipSuccess) return e;
  hipLaunchKernelGGL(part_off_kernel, dim3(pgrid), dim3(kRT), 0, s, ppos, plen, nlines, line_start, a.nparts,
                     d_part_off, d_info + 2);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipLaunchKernelGGL(write_batch_kernel, dim3(std::min<uint64_t>((nlines + 255) / 256, 4096)), dim3(kRT), 0, s, a.data,
                     n, nl, nlines, order, klen, vlen, flags, plen, ppos, out, out_cap);
  return hipGetLastError();
}

}  // namespace dgrep
