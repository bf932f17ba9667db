// job_arena.h — the device arena of the windowed whole job (job_arena.hip),
// shared with the runtime.
//
// Every pack flush and every window of a job encodes into its own 16-byte
// aligned buffer; the reduce wants every segment of the job back to back with
// no gap. One launch appends a flush's or a window's bytes to the arena at any
// byte offset and its rebased cell boundaries to the device segment table.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dgrep {

struct ArenaAppendArgs {
  const uint8_t* src = nullptr;  // 16-byte aligned, readable up to `total` rounded up to 16
  uint64_t total = 0;            // bytes to append
  uint8_t* arena = nullptr;      // 16-byte aligned base; [used, used + total) lies within its capacity
  uint64_t used = 0;
  // the cell boundaries of src: a pack's cell_off + 1 (cells entries, ascending,
  // the last one = total), or with running_max a window's partition ends
  // (nreduce entries: 0 for an empty partition, ascending otherwise, so cell i
  // ends at the largest entry up to i)
  const uint64_t* src_end = nullptr;
  uint64_t nend = 0;
  bool running_max = false;
  uint64_t* seg = nullptr;  // the table's entries behind the last one written: seg[i] = used + boundary i
};

// No byte before src or past its end rounded up to 16 is read; no byte outside
// arena[used, used + total) and no entry outside seg[0, nend) is written.
hipError_t arena_append(const ArenaAppendArgs& a, int num_cus, hipStream_t s);

}  // namespace dgrep
