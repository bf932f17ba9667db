// encode_batch.h — the partition + intermediate writer over the records of a
// batch scan (encode_batch.hip), shared with the runtime.
//
// Cell (s, p) = the bytes of mr-<s>-<p>: the json.Encoder lines of split s's
// KeyValues with ihash(Key) % nreduce == p, in line order. Cells are laid out
// split-major, then partition: cell c = s * nreduce + p occupies
// out[cell_off[c] : cell_off[c + 1]).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dgrep {

struct EncodeBatchArgs {
  const uint8_t* data;       // the packed buffer P (batch.h; 16-byte aligned)
  uint64_t n;                // its bytes (aligned dword reads never pass its last dword)
  const uint64_t* begin;     // [k + 1] (device): split s's first byte in P
  uint64_t k;                // splits
  const uint64_t* line_no;   // batch scan records: split-relative line and start
  const uint64_t* start;
  const uint64_t* len;
  const uint32_t* split;
  uint64_t count;            // < 2^32
  // the filename table (device): every name JSON-escaped (no quotes), concatenated
  const uint8_t* names;
  const uint64_t* name_off;   // [k + 1]: name s = names[name_off[s] : name_off[s + 1]), each below 2^31 bytes
  const uint32_t* name_hash;  // [k]: FNV-1a state after "filename[s] (line number #" (key_prefix_hash)
  uint32_t nreduce;           // k * nreduce < 2^32
};

// Encodes every record's KeyValue line into `out`, cell-major, line order
// inside a cell. d_cell_off (k * nreduce + 3 u64, device) receives the cells'
// offsets, entry k * nreduce being the total, then the number of values the
// chunked path took (escaped values of at least long_value bytes,
// encode_long.h) and the number of their chunks. Lines that would end past
// out_cap are not written. With scratch == nullptr or *scratch_bytes too small,
// only sets *scratch_bytes to the size needed. No byte outside a.data[0, a.n)
// is read by the chunked path.
hipError_t encode_batch(const EncodeBatchArgs& a, uint32_t long_value, void* scratch, size_t* scratch_bytes,
                        uint8_t* out, uint64_t out_cap, uint64_t* d_cell_off, hipStream_t s);

}  // namespace dgrep
