// reduce.hip — the grep reduce task on the GPU.
//
// Reference (map_reduce/worker.go):
//   readReduceInput (44-68): json.NewDecoder over each mr-<map>-<r> file, one
//     KeyValue per line (the lines encode.hip / writeMapOutput produced);
//   reduceDistinctKeys (22-42): sort.Sort(ByKey) -- NOT stable -- then one
//     reducef(key, values) per distinct key; the grep plugin's Reduce is
//     values[0] (application/grep.go:38-40), so the result is ONE of the
//     key's values (which one is unspecified for duplicate keys);
//   161-165: fmt.Sprintf("%v %v\n", k, v) per entry of a Go map, i.e. in
//     random order.
// Here: the concatenated input bytes sit in HBM; a newline select gives the
// lines; one thread per line decodes {"Key":"..","Value":".."} (JSON string
// escapes, \uXXXX incl. surrogate pairs -> UTF-8, raw invalid UTF-8 -> U+FFFD
// per byte) to measure the raw key and value and hash the raw key (FNV-1a 64);
// a radix sort of (hash, line) groups equal keys and an exact compare of the
// decoded keys inside each equal-hash run keeps the first line of every
// distinct key; a scan of the kept lines' output lengths places "key value\n";
// one wave per 64 kept lines writes them. Output order = input line order of
// the kept lines (one of the orders the reference can produce).
// Accepted input: lines of the compact two-field form
//     {"Key":"<json string>","Value":"<json string>"}\n
// byte for byte, with ANY JSON string encoding/json's decoder accepts (every
// escape it knows, either hex case, escaped or raw runes, invalid UTF-8); on
// such a line the key and value are exactly the decoder's. json.Encoder writes
// this form, and only its canonical spelling of it. Everything else -- white
// space, other field order or names, more fields, other JSON that the decoder
// would take -- is reported as malformed (DGREP_E_INVALID), never guessed.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include "reduce.h"
#include "reduce_common.h"

namespace dgrep {
namespace {
__global__ __launch_bounds__(kRT) void measure_kernel(const uint8_t* s, const uint64_t* nl, uint64_t nlines,
                                                      uint64_t* klen, uint64_t* vlen, uint64_t* kh, uint32_t* idx,
                                                      uint8_t* plain, unsigned long long* bad) {
  for (uint64_t j = uint64_t(blockIdx.x) * kRT + threadIdx.x; j < nlines; j += uint64_t(gridDim.x) * kRT) {
    const uint64_t a = j ? nl[j - 1] + 1 : 0, e = nl[j];
    bool pl;
    if (!parse_line<false>(s, a, e, nullptr, &klen[j], &vlen[j], &kh[j], &pl)) {
      atomicMin(bad, (unsigned long long)j);
      klen[j] = vlen[j] = 0;
      kh[j] = 0;
    }
    plain[j] = uint8_t(pl);
    idx[j] = uint32_t(j);
  }
}

// keep[line] = 1 unless an earlier line of the same equal-hash run has the
// identical raw key; sorted order by (hash, line). Equal escaped bytes mean
// equal keys (what json.Encoder writes is canonical, so its duplicates stop
// there); spellings that differ -- a hex escape for an ASCII byte, \/ for /,
// an escaped beside a raw rune, an invalid byte beside U+FFFD -- are decided
// on the decoded bytes, both keys decoded a unit at a time, whatever their
// length. With a malformed line in the input nothing is kept (and so nothing
// decoded again or written, whatever the malformed lines hold): the call fails.
__global__ __launch_bounds__(kRT) void dedupe_kernel(const uint8_t* s, const uint64_t* nl, const uint64_t* h_sorted,
                                                     const uint32_t* idx_sorted, uint64_t nlines, const uint64_t* klen,
                                                     uint64_t* out_len, const uint64_t* vlen,
                                                     const unsigned long long* bad) {
  const bool any_bad = *bad != ~0ull;
  for (uint64_t q = uint64_t(blockIdx.x) * kRT + threadIdx.x; q < nlines; q += uint64_t(gridDim.x) * kRT) {
    const uint32_t j = idx_sorted[q];
    bool keep = !any_bad;
    for (uint64_t p = q; keep && p-- > 0 && h_sorted[p] == h_sorted[q];) {
      const uint32_t k = idx_sorted[p];
      // different keys with one 64-bit hash take every "no" below: tests/test_gpu_reduce_collisions.py
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

// ---- writer: one WAVE per 64 kept lines ----------------------------------
// Lane l fetches line j0 + l's extents, then the wave walks the 64 lines and
// lane l builds output dwords (pos >> 2) + l + 64k of `key value\n`. A line
// that measure_kernel flagged plain (no escape and no coerced byte in either
// string, so its encoded length is 21 + raw key + raw value: the `{"Key":"`,
// `","Value":"`, `"}` frame) is a copy of two byte ranges: a dword wholly
// inside one range is one unaligned read (two aligned dwords + v_alignbyte);
// any other line is decoded by its own lane (parse_line). The lengths alone
// cannot tell the two apart: a coerced byte adds the two bytes that two
// short escapes take away.
__global__ __launch_bounds__(kRT) void write_kernel(const uint8_t* s, uint64_t n, const uint64_t* nl, uint64_t nlines,
                                                    const uint64_t* klen, const uint64_t* vlen,
                                                    const uint8_t* plain, const uint64_t* out_len,
                                                    const uint64_t* pos, uint8_t* out, uint64_t out_cap) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t nwaves = uint64_t(gridDim.x) * (kRT / 64);
  for (uint64_t j0 = (uint64_t(blockIdx.x) * (kRT / 64) + (threadIdx.x >> 6)) * 64u; j0 < nlines; j0 += nwaves * 64u) {
    const uint64_t jm = j0 + lane;
    uint64_t a = 0, e = 0, kl = 0, vl = 0, ol = 0, P = 0;
    int pl = 0;
    if (jm < nlines) {
      a = jm ? nl[jm - 1] + 1 : 0;
      e = nl[jm];
      ol = out_len[jm];
      P = pos[jm];
      kl = klen[jm];
      vl = vlen[jm];
      pl = plain[jm];
    }
    const uint32_t cnt = uint32_t(min(uint64_t(64), nlines - j0));
    for (uint32_t r = 0; r < cnt; ++r) {
      const uint64_t olr = __shfl(ol, int(r), 64), Pr = __shfl(P, int(r), 64);
      if (!olr || Pr + olr > out_cap) continue;
      const uint64_t ar = __shfl(a, int(r), 64), er = __shfl(e, int(r), 64);
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

__global__ __launch_bounds__(kRT) void count_kernel(const uint8_t* s, uint64_t n, unsigned long long* count) {
  uint64_t c = 0;
  for (uint64_t i = uint64_t(blockIdx.x) * kRT + threadIdx.x; i < n; i += uint64_t(gridDim.x) * kRT) c += s[i] == '\n';
  if (c) atomicAdd(count, (unsigned long long)c);
}

__global__ void total_kernel(const uint64_t* pos, const uint64_t* out_len, uint64_t nlines, uint64_t* total) {
  *total = pos[nlines - 1] + out_len[nlines - 1];
}

}  // namespace

hipError_t reduce_count_lines(const uint8_t* d_in, uint64_t n, uint64_t* d_count, hipStream_t s) {
  hipError_t e = hipMemsetAsync(d_count, 0, 8, s);
  if (e != hipSuccess || n == 0) return e;
  hipLaunchKernelGGL(count_kernel, dim3(grid_of(n)), dim3(kRT), 0, s, d_in, n,
                     reinterpret_cast<unsigned long long*>(d_count));
  return hipGetLastError();
}

hipError_t reduce_lines(const uint8_t* d_in, uint64_t n, uint64_t nlines, void* scratch, size_t* scratch_bytes,
                        uint8_t* out, uint64_t out_cap, uint64_t* d_info, hipStream_t s) {
  const uint64_t L = std::max<uint64_t>(nlines, 1);
  const uint64_t nblk = std::max<uint64_t>((n + kSeg - 1) / kSeg, 1);
  size_t sel_tmp = 0, sort_tmp = 0, scan_tmp = 0;
  hipError_t e = hipcub::DeviceScan::ExclusiveSum(nullptr, sel_tmp, (uint64_t*)nullptr, (uint64_t*)nullptr, nblk, s);
  if (e != hipSuccess) return e;
  if ((e = hipcub::DeviceRadixSort::SortPairs(nullptr, sort_tmp, (uint64_t*)nullptr, (uint64_t*)nullptr,
                                              (uint32_t*)nullptr, (uint32_t*)nullptr, L, 0, 64, s)) != hipSuccess)
    return e;
  if ((e = hipcub::DeviceScan::ExclusiveSum(nullptr, scan_tmp, (uint64_t*)nullptr, (uint64_t*)nullptr, L, s)) !=
      hipSuccess)
    return e;
  const size_t tmp = std::max({sel_tmp, sort_tmp, scan_tmp});
  const size_t need = a256(L * 8) * 7 + a256(L * 4) * 2 + a256(L) + a256(tmp) + 2 * a256(nblk * 8);
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
  uint64_t* pos = reinterpret_cast<uint64_t*>(take(L * 8));
  uint32_t* idx = reinterpret_cast<uint32_t*>(take(L * 4));
  uint32_t* idx_sorted = reinterpret_cast<uint32_t*>(take(L * 4));
  uint8_t* plain = take(L);
  void* t = take(tmp);
  uint64_t* blk_cnt = reinterpret_cast<uint64_t*>(take(nblk * 8));
  uint64_t* blk_off = reinterpret_cast<uint64_t*>(take(nblk * 8));

  // d_info: [0] lines found, [1] first malformed line (all ones: none), [2] output bytes
  if ((e = hipMemsetAsync(d_info, 0, 8, s)) != hipSuccess) return e;
  if ((e = hipMemsetAsync(d_info + 1, 0xff, 8, s)) != hipSuccess) return e;
  if ((e = hipMemsetAsync(d_info + 2, 0, 8, s)) != hipSuccess) return e;
  if (n == 0 || nlines == 0) return hipSuccess;
  size_t tb = tmp;
  hipLaunchKernelGGL(nl_count_kernel, dim3(nblk), dim3(kRT), 0, s, d_in, n, blk_cnt);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if ((e = hipcub::DeviceScan::ExclusiveSum(t, tb, blk_cnt, blk_off, nblk, s)) != hipSuccess) return e;
  hipLaunchKernelGGL(nl_write_kernel, dim3(nblk), dim3(kRT), 0, s, d_in, n, blk_off, nl);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipLaunchKernelGGL(nl_total_kernel, dim3(1), dim3(1), 0, s, blk_off, blk_cnt, nblk, d_info);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipLaunchKernelGGL(measure_kernel, dim3(grid_of(nlines)), dim3(kRT), 0, s, d_in, nl, nlines, klen, vlen, kh, idx,
                     plain, reinterpret_cast<unsigned long long*>(d_info + 1));
  if ((e = hipGetLastError()) != hipSuccess) return e;
  tb = tmp;
  if ((e = hipcub::DeviceRadixSort::SortPairs(t, tb, kh, kh_sorted, idx, idx_sorted, nlines, 0, 64, s)) != hipSuccess)
    return e;
  hipLaunchKernelGGL(dedupe_kernel, dim3(grid_of(nlines)), dim3(kRT), 0, s, d_in, nl, kh_sorted, idx_sorted, nlines,
                     klen, out_len, vlen, reinterpret_cast<const unsigned long long*>(d_info + 1));
  if ((e = hipGetLastError()) != hipSuccess) return e;
  tb = tmp;
  if ((e = hipcub::DeviceScan::ExclusiveSum(t, tb, out_len, pos, nlines, s)) != hipSuccess) return e;
  hipLaunchKernelGGL(write_kernel, dim3(std::min<uint64_t>((nlines + 255) / 256, 4096)), dim3(kRT), 0, s, d_in, n, nl,
                     nlines, klen, vlen, plain, out_len, pos, out, out_cap);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipLaunchKernelGGL(total_kernel, dim3(1), dim3(1), 0, s, pos, out_len, nlines, d_info + 2);
  return hipGetLastError();
}

}  // namespace dgrep
