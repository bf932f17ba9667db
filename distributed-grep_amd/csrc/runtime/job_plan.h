// job_plan.h — host arithmetic of the windowed whole job (dgrep_job_*).
//
// A job takes files in task order. A file the caller holds whole and that is
// at most one window long joins the current PACK: the packed buffer
// s_0 '\n' s_1 ... of dgrep_scan_batch, kept at or below window_bytes, flushed
// through one batch scan and one batch encode. Every other file -- longer than
// the window, or fed in pieces -- goes through the WINDOW route, after the pack
// was flushed, so the cells reach the arena in task order. Every flush adds
// k * nreduce segments to the arena's table, every window that completed a
// matching line adds nreduce. This header decides the routes and keeps the
// arena's offsets; it makes no HIP call, so a stand-alone program can drive it
// under a sanitizer (tests/job_c/job_plan_test.cpp).
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace dgrep {

enum JobRoute : uint32_t { kJobRoutePack = 0, kJobRouteWindow = 1 };

constexpr uint64_t kJobMaxSegments = uint64_t(1) << 32;  // the reduce's segment index is a u32
constexpr uint64_t kJobMaxLines = uint64_t(1) << 32;     // and so is its line index
constexpr uint64_t kJobArenaInitial = 4096;              // the arena's first allocation, bytes
constexpr uint64_t kJobSegInitial = 256;                 // the segment table's, entries

struct JobPlan {
  uint64_t window = 0;
  uint32_t nreduce = 0;
  // the open pack: its files and its bytes, separators included
  uint64_t pack_files = 0, pack_bytes = 0;
  // the arena: bytes used, segments in the table (the table holds nseg + 1 offsets)
  uint64_t used = 0, nseg = 0, lines = 0;
  // tallies (dgrep_job_stats)
  uint64_t files = 0, packs = 0, files_packed = 0, files_windowed = 0, rows = 0;
};

// what an arriving file asks for: flush the open pack first, then take `route`
struct JobStep {
  bool flush_first;
  JobRoute route;
  uint64_t pack_off;  // pack route: where the file's bytes lie in the packed buffer
};

// `streamed`: the file comes through begin / feed / end, its length unknown
inline JobRoute job_route(uint64_t window, uint64_t n, bool streamed) {
  return (streamed || n > window) ? kJobRouteWindow : kJobRoutePack;
}

// does a file of n <= window bytes join the open pack? The pack's bytes plus one
// separator per file after the first stay at or below the window; its cells
// below 2^32 (dgrep_map_partitions_batch's limit) and its files within a u32.
inline bool job_pack_fits(const JobPlan& p, uint64_t n) {
  if (p.pack_files == 0) return true;
  if (p.pack_bytes + 1 + n > p.window) return false;  // (no overflow: both terms are at most the window, <= 2^40)
  if ((p.pack_files + 1) * uint64_t(p.nreduce) >= kJobMaxSegments) return false;
  return p.pack_files + 1 <= UINT32_MAX;
}

// The next file, in task order. The caller flushes if asked (job_pack_flush),
// then either copies the file to pack_off (job_pack_push was done here) or
// streams it through the windows.
inline JobStep job_next_file(JobPlan* p, uint64_t n, bool streamed) {
  JobStep s;
  s.route = job_route(p->window, n, streamed);
  s.pack_off = 0;
  ++p->files;
  if (s.route == kJobRouteWindow) {
    s.flush_first = p->pack_files != 0;
    ++p->files_windowed;
    return s;
  }
  s.flush_first = !job_pack_fits(*p, n);
  ++p->files_packed;
  return s;
}

// the file's place in the pack, after the flush job_next_file may have asked for
inline uint64_t job_pack_push(JobPlan* p, uint64_t n) {
  const uint64_t off = p->pack_files ? p->pack_bytes + 1 : 0;  // behind the separator
  p->pack_bytes = off + n;
  ++p->pack_files;
  return off;
}

// closes the pack: returns its files (0: nothing to flush) and its bytes
inline uint64_t job_pack_flush(JobPlan* p, uint64_t* bytes) {
  const uint64_t k = p->pack_files;
  *bytes = p->pack_bytes;
  if (k) ++p->packs;
  p->pack_files = p->pack_bytes = 0;
  return k;
}

// One flush (rows = its files) or one window (rows = 1) appends `total` encoded
// bytes holding `lines` KeyValue lines as rows * nreduce segments. Returns the
// arena offset the bytes go to; false (nothing changed) if the job would pass
// the reduce's limits: *limit names which (0 segments, 1 lines).
inline bool job_append(JobPlan* p, uint64_t rows, uint64_t total, uint64_t lines, uint64_t* at, int* limit) {
  const uint64_t add = rows * uint64_t(p->nreduce);
  if (add >= kJobMaxSegments || p->nseg + add >= kJobMaxSegments) { *limit = 0; return false; }
  if (lines >= kJobMaxLines || p->lines + lines >= kJobMaxLines) { *limit = 1; return false; }
  *at = p->used;
  p->used += total;
  p->nseg += add;
  p->lines += lines;
  p->rows += rows;
  return true;
}

// geometric growth that keeps the contents: the new capacity for `need` units
inline uint64_t job_grow_cap(uint64_t cap, uint64_t need, uint64_t initial) {
  if (need <= cap) return cap;
  uint64_t c = cap ? 2 * cap : initial;
  return c < need ? need : c;
}

// The append kernel's split of `total` bytes going to arena offset `at` (the
// arena's base is 16-byte aligned): bytewise head up to the first aligned
// store, whole 16-byte stores, bytewise tail.
struct JobCopySplit {
  uint64_t head, vecs, tail;
};
inline JobCopySplit job_copy_split(uint64_t at, uint64_t total) {
  JobCopySplit s;
  s.head = (16 - (at & 15)) & 15;
  if (s.head > total) s.head = total;
  s.vecs = (total - s.head) / 16;
  s.tail = total - s.head - 16 * s.vecs;
  return s;
}

}  // namespace dgrep
