// reduce_batch.h — every reduce task of a job in one pass (reduce_batch.hip),
// shared with the runtime.
//
// Input: one buffer data[0:n) of KeyValue lines and a segment table
// seg_off[nseg + 1] (ascending, seg_off[0] = 0, seg_off[nseg] = n). Segment g
// belongs to partition g % nparts; partition p's reduce input is its segments
// in ascending g, concatenated (the mr-*-<p> files readReduceInput reads,
// map_reduce/worker.go:44-68). Segments sit back to back with no separator.
// R separate inputs: nseg = nparts = R. The batch writer's output as it is:
// nseg = nsplits * nreduce, nparts = nreduce, seg_off = its cell_off.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dgrep {

constexpr uint32_t kReduceBatchMaxParts = 65535;

struct ReduceBatchArgs {
  const uint8_t* data;      // 16-byte aligned when n > 0
  uint64_t n;
  const uint64_t* seg_off;  // [nseg + 1] (device)
  uint64_t nseg;            // < 2^32, a multiple of nparts
  uint32_t nparts;          // 1..65535
  uint64_t nlines;          // the '\n' in data[0:n) (reduce_count_lines), < 2^32
};

// d_info (device, 3 u64):
//   [0] lines found,
//   [1] the first malformed line, UINT64_MAX if none: partition << 34 | (0-based
//       line within the partition's input) << 1 | 1 for a line outside the
//       accepted form, ... | 0 for a segment that does not end in '\n' (its
//       unfinished last line); the lowest partition, then the lowest line,
//   [2] output bytes over all partitions (0 with a malformed line).
constexpr uint64_t reduce_batch_bad_part(uint64_t key) { return key >> 34; }
constexpr uint64_t reduce_batch_bad_line(uint64_t key) { return (key >> 1) & ((uint64_t(1) << 33) - 1); }

// For each partition, what reduce_lines writes for its concatenated input,
// the partitions in order in `out` (lines that would end past out_cap are not
// written). d_part_off (nparts + 1 u64, device): partition p's bytes are
// out[d_part_off[p] : d_part_off[p + 1]); d_lines_in (nparts u64, device): the
// KeyValue lines read for p. With a malformed line nothing is written and
// every offset is 0. With scratch == nullptr or *scratch_bytes too small, only
// sets *scratch_bytes to the size needed.
hipError_t reduce_batch(const ReduceBatchArgs& a, void* scratch, size_t* scratch_bytes, uint8_t* out,
                        uint64_t out_cap, uint64_t* d_part_off, uint64_t* d_lines_in, uint64_t* d_info,
                        hipStream_t s);

}  // namespace dgrep
