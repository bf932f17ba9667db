// encode.hip — the worker's partition + intermediate writer on the GPU.
//
// Reference (map_reduce/worker.go:78-109, writeMapOutput): for each reduce
// partition i, every KeyValue of the Map output with ihash(kv.Key) % nReduce
// == i is appended, in Map output order, to mr-<task>-<i> as the line
// json.NewEncoder(f).Encode(&kv) writes:
//     {"Key":<json string>,"Value":<json string>}\n
// ihash (worker.go:13-17) = FNV-1a 32 of the key & 0x7fffffff; the grep
// plugin's key is Sprintf("%s (line number #%v)", filename, line)
// (application/grep.go:25). Here the Map output is the scan's compacted
// records (line_no, start, len) over the HBM-resident split, so a partition's
// bytes are produced without ever building the KeyValue slice:
//   1. measure: per record, the key's partition (FNV-1a continued from the
//      host-hashed prefix "filename (line number #" over the decimal digits
//      and ')') and the encoded line's length (Go's JSON string escaping of the
//      value bytes, read from the split);
//   2. a stable radix sort of (partition, record) keeps line order inside a
//      partition; an exclusive scan of the sorted lengths gives each line's
//      byte offset; partition boundaries give each partition's byte range;
//   3. write: one wave per 64 lines emits them at their offsets.
// A value of at least `long_value` bytes that needs escaping is measured and
// written by the chunked path of encode_long.h, one workgroup per 16 KiB of it;
// its line's head and tail come from the line writers here.
// The kernels are built from the device functions of encode_pipeline.h, which
// the batch writer shares, as it does the host's sort, gather and scan.
// Algorithmic bytes: the matched lines' bytes read twice (measure, write) +
// the encoded output written once + ~40 B per record of sort/scan traffic.
#include "encode.h"
#include "encode_pipeline.h"

namespace dgrep {

uint64_t json_escape_host(const uint8_t* s, uint64_t n, uint8_t* out) {
  return out ? json_body<true>(s, n, out) : json_body<false>(s, n, nullptr);
}

uint32_t key_prefix_hash(const uint8_t* filename, uint64_t fn) {
  uint32_t h = 2166136261u;
  for (uint64_t i = 0; i < fn; ++i) h = fnv_step(h, filename[i]);
  const char* mid = " (line number #";
  for (int i = 0; mid[i]; ++i) h = fnv_step(h, uint8_t(mid[i]));
  return h;
}

namespace {
// Per record (one thread each): the key's partition and the encoded line's
// length ASSUMING a plain value (nothing to escape); encode_values_kernel
// corrects the length of the rare values that need escaping.
__global__ __launch_bounds__(kEncThreads) void encode_measure_kernel(EncodeArgs a, uint16_t* part, uint32_t* idx,
                                                                     uint64_t* enc_len, uint32_t* nchunks) {
  if (blockIdx.x == 0 && threadIdx.x == 0) nchunks[a.count] = 0;  // the scan's last entry: the total
  for (uint64_t i = uint64_t(blockIdx.x) * kEncThreads + threadIdx.x; i < a.count;
       i += uint64_t(gridDim.x) * kEncThreads) {
    uint8_t d[20];
    const uint32_t nd = digits_of(a.line_no[i], d);
    part[i] = uint16_t(key_ihash(a.key_hash0, d, nd) % a.nreduce);
    idx[i] = uint32_t(i);
    enc_len[i] = plain_line_len(a.fname_json_len, nd, a.len[i]);
  }
}

// One WAVE per record (value_needs_escape); a value with anything to escape
// gets its exact encoded length from json_body (lane 0) if it is short, its
// chunk count if it is long (value_measured). lo = the buffer's address & 15.
__global__ __launch_bounds__(kEncThreads) void encode_values_kernel(EncodeArgs a, uint32_t long_value, uint64_t lo,
                                                                    uint64_t* enc_len, uint32_t* nchunks) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t waves = uint64_t(gridDim.x) * kEncWaves;
  for (uint64_t i = uint64_t(blockIdx.x) * kEncWaves + (threadIdx.x >> 6); i < a.count; i += waves) {
    const uint64_t st = a.start[i], e = st + a.len[i];
    const bool escaped = value_needs_escape(a.data, a.n, st, e, lane, e - st >= long_value);  // wave-uniform
    value_measured(a.data, st, e, lo + st, escaped, long_value, lane, enc_len + i, nchunks + i);
  }
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

// One WAVE per 64 output lines (sorted order j0 .. j0 + 63). Lane l first
// fetches line j0 + l's record (coalesced: idx, pos, length, then the record)
// and writes its line number's digits to the wave's LDS row; then the wave
// walks the 64 lines, each broadcast from its lane, and writes it
// (write_plain_line, the constant head from LDS). A value that needs escaping
// is written by its own lane alone behind that loop (write_line_thread); a long
// one's bytes are left to the chunk pass, which finds their place in val_pos[record].
__global__ __launch_bounds__(kEncThreads) void encode_write_kernel(EncodeArgs a, const uint32_t* idx,
                                                                   const uint64_t* pos, const uint64_t* len_sorted,
                                                                   uint32_t* nchunks, uint64_t* val_pos, uint8_t* out,
                                                                   uint64_t out_cap) {
  __shared__ uint8_t head[kHeadMax];
  __shared__ uint8_t dig[kEncWaves][64][20];
  const uint32_t F = a.fname_json_len, A = 8u + F + 15u;  // head bytes (host guarantees A <= kHeadMax)
  for (uint32_t k = threadIdx.x; k < A; k += kEncThreads) head[k] = head_byte(a.fname_json, F, k);
  __syncthreads();
  const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
  const uint64_t nwaves = uint64_t(gridDim.x) * kEncWaves;
  for (uint64_t j0 = (uint64_t(blockIdx.x) * kEncWaves + wv) * 64u; j0 < a.count; j0 += nwaves * 64u) {
    const uint64_t jm = j0 + lane;
    uint64_t P = 0, T = 0, st = 0, L = 0, i = 0;
    uint32_t nd = 0;
    if (jm < a.count) {
      i = idx[jm];
      P = pos[jm];
      T = len_sorted[jm];
      st = a.start[i];
      L = a.len[i];
      uint8_t d[20];
      nd = digits_of(a.line_no[i], d);
      for (uint32_t k = 0; k < nd; ++k) dig[wv][lane][k] = d[k];
    }
    wave_publish_lds();
    const uint32_t cnt = uint32_t(min(uint64_t(64), a.count - j0));
    for (uint32_t r = 0; r < cnt; ++r) {
      const uint64_t Pr = __shfl(P, int(r), 64), Tr = __shfl(T, int(r), 64);
      const uint64_t str = __shfl(st, int(r), 64), Lr = __shfl(L, int(r), 64);
      const uint32_t ndr = uint32_t(__shfl(int(nd), int(r), 64));
      if (Pr + Tr > out_cap) continue;
      if (Tr != plain_line_len(F, ndr, Lr)) continue;  // escaped value (wave-uniform, rare): below
      write_plain_line(a.data, a.n, out, Pr, Tr, str, Lr, A, ndr, dig[wv][r], lane,
                       [&](uint64_t o) -> uint32_t { return head[o]; });
    }
    // the escaped lines, each by its own lane, behind the loop so that this path's registers are not the loop's
    if (jm < a.count && P + T <= out_cap && T != plain_line_len(F, nd, L))
      write_line_thread(a.fname_json, F, a.line_no[i], a.data, a.start[i], a.len[i], out, P, T, nchunks, val_pos, i);
    __builtin_amdgcn_wave_barrier();  // the LDS digit row is rewritten next round
  }
}

// the per-thread writer for file names whose head does not fit kHeadMax
__global__ __launch_bounds__(kEncThreads) void encode_write_thread_kernel(EncodeArgs a, const uint32_t* idx,
                                                                          const uint64_t* pos,
                                                                          const uint64_t* len_sorted,
                                                                          uint32_t* nchunks, uint64_t* val_pos,
                                                                          uint8_t* out, uint64_t out_cap) {
  for (uint64_t j = uint64_t(blockIdx.x) * kEncThreads + threadIdx.x; j < a.count;
       j += uint64_t(gridDim.x) * kEncThreads) {
    if (pos[j] + len_sorted[j] > out_cap) continue;
    const uint64_t i = idx[j];
    write_line_thread(a.fname_json, a.fname_json_len, a.line_no[i], a.data, a.start[i], a.len[i], out, pos[j],
                      len_sorted[j], nchunks, val_pos, i);
  }
}

// where record i's value lies (encode_long.h): start[i], as a position
struct ResidentLoc {
  const uint64_t* start;
  uint64_t lo;
  __device__ uint64_t operator()(uint64_t i) const { return lo + start[i]; }
};
}  // namespace

hipError_t encode_partitions(const EncodeArgs& a, uint32_t long_value, void* scratch, size_t* scratch_bytes,
                             uint8_t* out, uint64_t out_cap, uint64_t* d_bounds, hipStream_t s) {
  const uint64_t n = a.count, max_chunks = long_max_chunks(a.n, n, long_value);
  const int end_bit = key_bits(a.nreduce);
  size_t tmp = 0, long_tmp = 0;
  hipError_t e = sort_gather_scan_tmp<uint16_t>(n, end_bit, &tmp, s);
  if (e != hipSuccess) return e;
  if ((e = long_scan_tmp(n, &long_tmp, s)) != hipSuccess) return e;
  tmp = std::max(tmp, long_tmp);
  const size_t need = LineTables<uint16_t>::bytes(n) + LongTables::bytes(n, max_chunks) + align256(tmp);
  if (!scratch || *scratch_bytes < need) {
    *scratch_bytes = need;
    return hipSuccess;
  }
  ScratchCarver c{static_cast<uint8_t*>(scratch)};
  const LineTables<uint16_t> q(c, n);
  const LongTables lq(c, n, max_chunks);
  void* t = c.take<uint8_t>(tmp);
  uint64_t* val_pos = q.enc_len;  // enc_len is dead once gathered into len_sorted
  const LongSpan sp = long_span(a.data, a.n);
  const ResidentLoc loc{a.start, sp.lo};

  e = hipMemsetAsync(d_bounds, 0, (2 * size_t(a.nreduce) + 3) * 8, s);
  if (e != hipSuccess || n == 0) return e;
  hipLaunchKernelGGL(encode_measure_kernel, dim3(grid_for(n)), dim3(kEncThreads), 0, s, a, q.key_in, q.idx_in,
                     q.enc_len, lq.nchunks);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipLaunchKernelGGL(encode_values_kernel, dim3(wave_grid_for(n)), dim3(kEncThreads), 0, s, a, long_value, sp.lo,
                     q.enc_len, lq.nchunks);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if ((e = long_measure(sp, loc, a.len, n, lq, q.enc_len, d_bounds + 2 * size_t(a.nreduce) + 1, t, tmp, s)) !=
      hipSuccess)
    return e;
  if ((e = sort_gather_scan(q, n, end_bit, t, tmp, s)) != hipSuccess) return e;
  hipLaunchKernelGGL(bounds_kernel, dim3(grid_for(n)), dim3(kEncThreads), 0, s, q.key_out, q.pos, q.len_sorted, n,
                     a.nreduce, d_bounds);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if (8u + a.fname_json_len + 15u <= kHeadMax)
    hipLaunchKernelGGL(encode_write_kernel, dim3(wave64_grid_for(n)), dim3(kEncThreads), 0, s, a, q.idx_out, q.pos,
                       q.len_sorted, lq.nchunks, val_pos, out, out_cap);
  else
    hipLaunchKernelGGL(encode_write_thread_kernel, dim3(grid_for(n)), dim3(kEncThreads), 0, s, a, q.idx_out, q.pos,
                       q.len_sorted, lq.nchunks, val_pos, out, out_cap);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  return long_write(sp, loc, a.len, n, lq, val_pos, out, s);
}

}  // namespace dgrep
