// batch.h — many splits in one scan (batch.hip), shared with the runtime.
//
// The packed buffer P = s_0 '\n' s_1 '\n' ... '\n' s_{k-1} (one '\n' between
// consecutive splits, none after the last) splits into exactly the lines of
// the k splits, in order, so one ordinary scan of P finds every split's
// matching lines with P-wide line numbers and starts. These kernels rebase
// them per split. begin[i] = sum_{j<i} (len_j + 1) is split i's first byte in
// P; region i = [begin[i], begin[i+1]) is the split plus its separator, and
// begin[k] = n + 1 closes the last region (which has no separator).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dgrep {

struct BatchArgs {
  const uint8_t* data;    // P (16-byte aligned; aligned 16-B reads never pass its last granule)
  uint64_t n;             // bytes of P
  const uint64_t* begin;  // [k + 1] (device), strictly increasing, begin[0] = 0, begin[k] = n + 1
  uint64_t k;             // splits, 1 .. 2^32 - 1
  // [k], zeroed before batch_split_newlines: '\n' per region, then (in place)
  // the lines before split i = first_line[i] - 1
  unsigned long long* lines;
  unsigned long long* block_sums;  // [kBatchScanBlocks] scratch of the scan over `lines`
  // lowest split whose separator byte P[begin[i+1] - 1] is not '\n' (set to
  // UINT64_MAX before the call; stays so for a well-formed P)
  unsigned long long* bad_split;
};
constexpr int kBatchScanBlocks = 1024;

// lines[i] = number of '\n' in P[0 : begin[i]) for every split, and the
// separator check. Reads every byte of P once, whatever the split sizes.
hipError_t batch_split_newlines(const BatchArgs& a, int num_cus, hipStream_t s);

// split_begin[s] = first record whose P-wide start is >= begin[s] (s < k),
// split_begin[k] = nrec: split s owns records [split_begin[s], split_begin[s+1]).
// `start` holds the scan's P-wide starts: run it BEFORE batch_rebase.
hipError_t batch_split_ranges(const BatchArgs& a, const uint64_t* start, uint64_t nrec, uint64_t* split_begin,
                              int num_cus, hipStream_t s);

// In place over the scan's first nrec records (ascending start): split[r] =
// the split holding start[r]; line_no[r] and start[r] become relative to it.
hipError_t batch_rebase(const BatchArgs& a, uint64_t* line_no, uint64_t* start, uint32_t* split, uint64_t nrec,
                        int num_cus, hipStream_t s);

}  // namespace dgrep
