// window.h — a split consumed in windows (window.hip), shared with the runtime.
//
// The stream's bytes arrive in windows; the device holds two window buffers.
// `fill` = the carried tail (the unfinished line of the window before) followed
// by the window's new bytes, at the start of one buffer. With cut = the position
// of the last '\n' in fill, fill[0 : cut) holds exactly the lines this window
// completed: strings.Split of that region is their list (the separator at cut
// is excluded, so no phantom empty line appears). One ordinary scan of the
// region finds their matching lines with region-wide line numbers and starts;
// these kernels find the cut, rebase the records by the stream's running bases
// and gather the matching lines' bytes. fill[cut + 1 :) is carried to the front
// of the other buffer. None of them touches the scan kernels.
//
// A window with no '\n' completes no line: all of fill is carried, so the
// device footprint is bounded by the window plus the longest unfinished line,
// not by the split. A bounded stream (carry.h) folds such a window into the
// line's DFA state instead, so that even one giant line stays bounded.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dgrep {

constexpr int kCutBlocks = 2048;  // most workgroups of the cut pass

// cut[0] = 1 + the position of the last '\n' in data[0 : n) (0: none), cut[1] =
// the number of '\n' in data[0 : n), cut[2] = 1 + the position of the first
// '\n' in data[from : n) (0: none) -- with from = the carried tail's length,
// the end of the line the tail began. One streaming read. `data` is 16-byte
// aligned and its allocation covers n rounded up to 16 bytes (bytes at or past
// n are read and ignored). partials: 3 * kCutBlocks entries of scratch.
hipError_t window_cut(const uint8_t* data, uint64_t n, uint64_t from, unsigned long long* partials,
                      unsigned long long* cut, int num_cus, hipStream_t s);

// dst_*[r] = the window's record r moved to the stream's coordinates, r < nrec:
// line_no + line_base, start + byte_base, len as it is.
hipError_t window_rebase_append(const uint64_t* line_no, const uint64_t* start, const uint64_t* len, uint64_t nrec,
                                uint64_t line_base, uint64_t byte_base, uint64_t* dst_line, uint64_t* dst_start,
                                uint64_t* dst_len, int num_cus, hipStream_t s);

// The matching lines' bytes, in record order, contiguous in `values`:
// record r's line = values[off[r] : off[r + 1]) with off = the exclusive scan
// of len. value_off[r + 1] = value_base + off[r + 1] for r < nrec (the caller
// owns value_off[0], the end of the records before). start / len are the
// window's own records (offsets into data). *total (device) = off[nrec].
// Call with scratch == nullptr to get *scratch_bytes.
struct GatherArgs {
  const uint8_t* data;
  const uint64_t* start;
  const uint64_t* len;
  uint64_t nrec;  // 1 .. 2^32 - 1
  uint64_t value_base;
  uint64_t* value_off;  // nrec + 1 entries; [0] is not written
  uint8_t* values;      // at least sum(len) bytes
  unsigned long long* total;
};
hipError_t window_gather(const GatherArgs& a, void* scratch, size_t* scratch_bytes, int num_cus, hipStream_t s);

}  // namespace dgrep
