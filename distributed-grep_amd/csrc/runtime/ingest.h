// ingest.h — host bytes -> HBM through the pinned staging ring.
//
// The source is P as pack_pieces.h describes it: k buffers data[i][0 : n[i]),
// with one '\n' between them when `sep`; a single buffer is k = 1. Piece p of P
// is assembled by the CPU threads into staging buffer p % B, once the DMA that
// last read that buffer has finished, and then DMA'd on the copy stream: the
// CPU copy of piece p + 1 overlaps the DMA of piece p.
//
// The ring has ONE reuse rule: a staging buffer is refilled only after its own
// event, recorded behind its last DMA, is done. An event never recorded, or
// complete, returns at once. No caller has to know what another one left in
// flight. Everything else -- what the first DMA waits for, who waits for the
// last one -- is the caller's completion contract (dgrep_runtime.hip:
// ingest_resident drains the copy stream, win_ingest returns with DMAs queued).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "device_buf.h"
#include "pack_pieces.h"

namespace dgrep {

struct IngestRing {
  // dgrep_set_ingest: `threads` CPU threads copy into one of `bufs` pinned
  // buffers of `chunk` bytes (chunk 0: always the direct path)
  size_t chunk = size_t(64) << 20;
  int bufs = 4;
  int threads = 4;
  Stream copy_stream;
  std::vector<PinnedBuf<uint8_t>> h_stage;
  std::vector<Event> ev_stage;
  size_t stage_bytes = 0;
  int last = 0;                    // the staging buffer of the last DMA queued
  std::vector<uint8_t> bat_stage;  // the direct path's one staging buffer (k > 1)
  const char* what = "";           // the HIP call that failed
};

#define DGREP_INGEST_HIP(expr)                    \
  do {                                            \
    const hipError_t e_ = (expr);                 \
    if (e_ != hipSuccess) return r->what = #expr, e_; \
  } while (0)

// chunk 0, or fewer than 4 MiB: one copy, no ring
inline bool ingest_direct(const IngestRing& r, size_t total) { return r.chunk == 0 || total < (size_t(4) << 20); }

// The direct path: one hipMemcpyAsync on `stream`, straight from the caller's
// pageable bytes when k == 1, else from P assembled in bat_stage.
inline hipError_t ingest_direct_copy(IngestRing* r, const uint8_t* const* data, const size_t* n, size_t k, bool sep,
                                     uint8_t* dst, size_t total, hipStream_t stream) {
  const uint8_t* src = data[0];
  if (k > 1) {
    r->bat_stage.resize(total);
    PackCursor cur;
    std::vector<PackSeg> segs;
    pack_piece_segments(n, k, &cur, total, &segs, sep);
    for (const PackSeg& s : segs) pack_copy_segment(data, s, r->bat_stage.data(), std::max(1, r->threads));
    src = r->bat_stage.data();
  }
  DGREP_INGEST_HIP(hipMemcpyAsync(dst, src, total, hipMemcpyHostToDevice, stream));
  return hipSuccess;
}

// The ring as the settings ask for it: the copy stream, and the staging buffers
// with their events, reallocated (behind the DMAs in flight) when the chunk
// size or the count changed.
inline hipError_t ingest_ring(IngestRing* r) {
  DGREP_INGEST_HIP(r->copy_stream.create());
  const size_t S = r->chunk, B = size_t(std::max(2, r->bufs));
  if (r->stage_bytes == S && r->h_stage.size() == B) return hipSuccess;
  DGREP_INGEST_HIP(hipStreamSynchronize(r->copy_stream));
  r->stage_bytes = 0;
  r->h_stage = std::vector<PinnedBuf<uint8_t>>(B);
  r->ev_stage = std::vector<Event>(B);
  for (size_t b = 0; b < B; ++b) {
    DGREP_INGEST_HIP(r->h_stage[b].alloc(S));
    DGREP_INGEST_HIP(r->ev_stage[b].create(hipEventDisableTiming));
  }
  r->stage_bytes = S;
  return hipSuccess;
}

// The piece loop: the `total` bytes of P to dst, queued on the copy stream
// through the ring (ingest_ring has run). Returns with the last DMA queued and
// r->last naming its buffer.
inline hipError_t ingest_pieces(IngestRing* r, const uint8_t* const* data, const size_t* n, size_t k, bool sep,
                                uint8_t* dst, size_t total) {
  const size_t S = r->stage_bytes, B = r->h_stage.size();
  const int T = std::max(1, r->threads);
  PackCursor cur;
  std::vector<PackSeg> segs;
  for (size_t off = 0, p = 0; off < total; off += S, ++p) {
    const int b = int(p % B);
    const size_t len = std::min(S, total - off);
    DGREP_INGEST_HIP(hipEventSynchronize(r->ev_stage[b]));  // buffer b's last DMA is done (or it never had one)
    pack_piece_segments(n, k, &cur, len, &segs, sep);
    for (const PackSeg& s : segs) pack_copy_segment(data, s, r->h_stage[b], T);
    DGREP_INGEST_HIP(hipMemcpyAsync(dst + off, r->h_stage[b], len, hipMemcpyHostToDevice, r->copy_stream));
    DGREP_INGEST_HIP(hipEventRecord(r->ev_stage[b], r->copy_stream));
    r->last = b;
  }
  return hipSuccess;
}

#undef DGREP_INGEST_HIP

}  // namespace dgrep
