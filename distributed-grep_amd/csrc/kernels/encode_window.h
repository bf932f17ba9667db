// encode_window.h — the partition + intermediate writer over one WINDOW of a
// streamed split (encode_window.hip), shared with the runtime.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "encode.h"

namespace dgrep {

// A long escaped value is cut into chunks of kLongChunk bytes, one workgroup
// each (measured: DESIGN §3.13). A multiple of kLongStep.
#ifndef DGREP_LONG_CHUNK
#define DGREP_LONG_CHUNK 16384
#endif
constexpr uint32_t kLongStep = 4096;  // 256 lanes x 16 bytes: one workgroup step
constexpr uint32_t kLongChunk = DGREP_LONG_CHUNK;
static_assert(kLongChunk % kLongStep == 0 && kLongChunk >= kLongStep, "whole workgroup steps");
// dgrep_set_long_value(0): the value length from which an escaped value takes
// the chunked path. Measured: the chunked path is the faster one
// from 256 bytes on, the smallest length the setter admits, for one value alone
// and for a window full of them; so the default is that floor.
constexpr uint32_t kLongValueDefault = 256;
// The same default for the resident and the batch writer (encode_long.h), whose
// one-lane path runs every escaped line's lane at once: measured (DESIGN §3.13,
// round 17), a split full of escaped values is faster by one lane each below 768
// bytes a value and by chunks from there on.
constexpr uint32_t kLongValueResidentDefault = 768;

struct WindowEncodeArgs {
  EncodeArgs e;         // data = the window buffer, records in the WINDOW's coordinates
  uint64_t line_base;   // lines of the stream before this window: added where the line number is printed or hashed
  uint32_t long_value;  // an escaped value of at least this many bytes takes the chunked path
};

// encode_partitions (encode.h) for one window. d_bounds has 2 * nreduce + 2
// entries: the last one is the number of values the chunked path took.
// The buffer behind e.data is readable up to e.n rounded up to 16 bytes
// (window.h's guarantee); no read falls outside that.
hipError_t encode_window_partitions(const WindowEncodeArgs& a, void* scratch, size_t* scratch_bytes, uint8_t* out,
                                    uint64_t out_cap, uint64_t* d_bounds, hipStream_t s);

}  // namespace dgrep
