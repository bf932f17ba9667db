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
// A record's value lies at P[begin[split] + start : + len). A value of at least
// `long_value` bytes that needs escaping takes the chunked path of
// encode_long.h, as in encode.hip.
#include "encode_batch.h"
#include "encode_pipeline.h"

namespace dgrep {

namespace {
__global__ __launch_bounds__(kEncThreads) void batch_measure_kernel(EncodeBatchArgs a, uint32_t* cell, uint32_t* idx,
                                                                    uint64_t* enc_len, uint32_t* nchunks,
                                                                    uint64_t* stats) {
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    nchunks[a.count] = 0;  // the scan's last entry: the total
    stats[0] = stats[1] = 0;  // long_fix_kernel counts the long values and their chunks here
  }
  for (uint64_t i = uint64_t(blockIdx.x) * kEncThreads + threadIdx.x; i < a.count;
       i += uint64_t(gridDim.x) * kEncThreads) {
    const uint32_t sp = a.split[i];
    uint8_t d[20];
    const uint32_t nd = digits_of(a.line_no[i], d);
    cell[i] = sp * a.nreduce + key_ihash(a.name_hash[sp], d, nd) % a.nreduce;  // < k * nreduce < 2^32
    idx[i] = uint32_t(i);
    enc_len[i] = plain_line_len(uint32_t(a.name_off[sp + 1] - a.name_off[sp]), nd, a.len[i]);
  }
}

// One WAVE per record (value_needs_escape over the value's bytes in P); a value
// with anything to escape gets its exact encoded length from json_body (lane
// 0) if it is short, its chunk count if it is long (value_measured). lo = P's
// address & 15.
__global__ __launch_bounds__(kEncThreads) void batch_values_kernel(EncodeBatchArgs a, uint32_t long_value, uint64_t lo,
                                                                   uint64_t* enc_len, uint32_t* nchunks) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t waves = uint64_t(gridDim.x) * kEncWaves;
  for (uint64_t i = uint64_t(blockIdx.x) * kEncWaves + (threadIdx.x >> 6); i < a.count; i += waves) {
    const uint64_t st = a.begin[a.split[i]] + a.start[i], e = st + a.len[i];
    const bool escaped = value_needs_escape(a.data, a.n, st, e, lane, e - st >= long_value);  // wave-uniform
    value_measured(a.data, st, e, lo + st, escaped, long_value, lane, enc_len + i, nchunks + i);
  }
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

// One WAVE per 64 output lines (sorted order j0 .. j0 + 63), as the resident
// writer's encode_write_kernel (encode.hip): lane l fetches line j0 + l's
// record and writes its line number's digits to the wave's LDS row; then the
// wave walks the 64 lines, each broadcast from its lane, and writes it
// (write_plain_line).
// The head differs per line here: it comes from the wave's LDS row when all the
// wave's lines share a split and the head fits the row (`staged`,
// wave-uniform), else from the filename table. A line that would end past
// out_cap is skipped. A long escaped value's bytes are left to the chunk pass,
// which finds their place in val_pos[record].
__global__ __launch_bounds__(kEncThreads) void batch_write_kernel(EncodeBatchArgs a, const uint32_t* idx,
                                                                  const uint64_t* pos, const uint64_t* len_sorted,
                                                                  uint32_t* nchunks, uint64_t* val_pos, uint8_t* out,
                                                                  uint64_t out_cap) {
  __shared__ uint8_t head[kEncWaves][kHeadMax];
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
    const bool staged = __ballot(jm < a.count && sp != sp0) == 0ull && 8u + F0 + 15u <= kHeadMax;
    if (staged) {
      for (uint32_t k = lane; k < 8u + F0 + 15u; k += 64u) head[wv][k] = head_byte(a.names + no0, F0, k);
    }
    wave_publish_lds();
    const uint32_t cnt = uint32_t(min(uint64_t(64), a.count - j0));
    for (uint32_t r = 0; r < cnt; ++r) {
      const uint64_t Pr = __shfl(P, int(r), 64), Tr = __shfl(T, int(r), 64);
      const uint64_t srcr = __shfl(src, int(r), 64), Lr = __shfl(L, int(r), 64);
      const uint64_t nor = __shfl(no, int(r), 64);
      const uint32_t ndr = uint32_t(__shfl(int(nd), int(r), 64)), Fr = uint32_t(__shfl(int(F), int(r), 64));
      if (Pr + Tr > out_cap) continue;
      if (Tr != plain_line_len(Fr, ndr, Lr)) continue;  // escaped value (wave-uniform, rare): below
      write_plain_line(a.data, a.n, out, Pr, Tr, srcr, Lr, 8u + Fr + 15u, ndr, dig[wv][r], lane,
                       [&](uint64_t o) -> uint32_t {
                         if (staged) return head[wv][o];
                         return head_byte(a.names + nor, Fr, o);
                       });
    }
    // the escaped lines, each by its own lane, behind the loop so that this path's registers are not the loop's
    if (jm < a.count && P + T <= out_cap && T != plain_line_len(F, nd, L))
      write_line_thread(a.names + no, F, a.line_no[i], a.data, src, L, out, P, T, nchunks, val_pos, i);
    __builtin_amdgcn_wave_barrier();  // the LDS rows are rewritten next round
  }
}

// where record i's value lies (encode_long.h): begin[split[i]] + start[i], as a position
struct BatchLoc {
  const uint64_t* begin;
  const uint32_t* split;
  const uint64_t* start;
  uint64_t lo;
  __device__ uint64_t operator()(uint64_t i) const { return lo + begin[split[i]] + start[i]; }
};
}  // namespace

hipError_t encode_batch(const EncodeBatchArgs& a, uint32_t long_value, void* scratch, size_t* scratch_bytes,
                        uint8_t* out, uint64_t out_cap, uint64_t* d_cell_off, hipStream_t s) {
  const uint64_t n = a.count, cells = a.k * uint64_t(a.nreduce), max_chunks = long_max_chunks(a.n, n, long_value);
  const int end_bit = key_bits(cells);
  size_t tmp = 0, long_tmp = 0;
  hipError_t e = sort_gather_scan_tmp<uint32_t>(n, end_bit, &tmp, s);
  if (e != hipSuccess) return e;
  if ((e = long_scan_tmp(n, &long_tmp, s)) != hipSuccess) return e;
  tmp = std::max(tmp, long_tmp);
  const size_t need = LineTables<uint32_t>::bytes(n) + LongTables::bytes(n, max_chunks) + align256(tmp);
  if (!scratch || *scratch_bytes < need) {
    *scratch_bytes = need;
    return hipSuccess;
  }
  ScratchCarver c{static_cast<uint8_t*>(scratch)};
  const LineTables<uint32_t> q(c, n);
  const LongTables lq(c, n, max_chunks);
  void* t = c.take<uint8_t>(tmp);
  uint64_t* val_pos = q.enc_len;  // enc_len is dead once gathered into len_sorted
  uint64_t* stats = d_cell_off + cells + 1;
  const LongSpan sp = long_span(a.data, a.n);
  const BatchLoc loc{a.begin, a.split, a.start, sp.lo};

  if (n == 0) return hipMemsetAsync(d_cell_off, 0, (cells + 3) * 8, s);
  hipLaunchKernelGGL(batch_measure_kernel, dim3(grid_for(n)), dim3(kEncThreads), 0, s, a, q.key_in, q.idx_in,
                     q.enc_len, lq.nchunks, stats);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipLaunchKernelGGL(batch_values_kernel, dim3(wave_grid_for(n)), dim3(kEncThreads), 0, s, a, long_value, sp.lo,
                     q.enc_len, lq.nchunks);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if ((e = long_measure(sp, loc, a.len, n, lq, q.enc_len, stats, t, tmp, s)) != hipSuccess) return e;
  if ((e = sort_gather_scan(q, n, end_bit, t, tmp, s)) != hipSuccess) return e;
  hipLaunchKernelGGL(batch_cell_off_kernel, dim3(grid_for(cells + 1)), dim3(kEncThreads), 0, s, q.key_out, q.pos,
                     q.len_sorted, n, cells, d_cell_off);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipLaunchKernelGGL(batch_write_kernel, dim3(wave64_grid_for(n)), dim3(kEncThreads), 0, s, a, q.idx_out, q.pos,
                     q.len_sorted, lq.nchunks, val_pos, out, out_cap);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  return long_write(sp, loc, a.len, n, lq, val_pos, out, s);
}

}  // namespace dgrep
