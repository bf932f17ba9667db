// dgrep_runtime.hip — device contexts, DFA upload, split scanning (C ABI).
//
// This is the native runtime under the grep plugin's Map (application/grep.go:13-36):
// dgrep_scan replaces the strings.Split + per-line regexp.Match loop
// (grep.go:17-29) for one split. Everything here is fail-stop: a HIP error is
// returned as DGREP_E_HIP with its message in dgrep_last_error; there is no
// CPU fallback path.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <map>
#include <chrono>
#include <string>
#include <thread>
#include <vector>

#include <unistd.h>

#include "../../../include/dgrep.h"
#include "../../../include/dgrep_blob.h"
#include "../kernels/batch.h"
#include "../kernels/carry.h"
#include "../kernels/encode.h"
#include "../kernels/encode_batch.h"
#include "../kernels/encode_window.h"
#include "../kernels/job_arena.h"
#include "../kernels/reduce.h"
#include "../kernels/reduce_batch.h"
#include "../kernels/scan_common.h"
#include "../kernels/synth.h"
#include "../kernels/window.h"
#include "device_buf.h"
#include "ingest.h"
#include "job_plan.h"
#include "pack_pieces.h"
#include "pattern_image.h"

// DFAs of at most this many states use the Sheng stepper (8 = its limit; 0
// sends every DFA of <= 256 states to the table stepper). The stand-alone
// builder takes the same default from pattern_layout.h, included above.
#ifndef DGREP_SHENG_MAX_STATES
#define DGREP_SHENG_MAX_STATES 8
#endif
// matching-line records per resident thread of the HBM spill area the
// one-chunk-per-lane steppers move full LDS slots to (0: no spilling)
#ifndef DGREP_SPILL_RECORDS
#define DGREP_SPILL_RECORDS 240
#endif
// A/B knobs (shipped: 1, 1): park long lines at all (0: a lane reads its last
// line to its end), and the Sheng stepper's chunk maps (0: Sheng parks at 2 C
// and resolves through the per-chunk '\n' counts like the other steppers)
#ifndef DGREP_PARK
#define DGREP_PARK 1
#endif
// A/B knob: cap on the scan's resident workgroups per CU (the grid)
#ifndef DGREP_MAX_WG_PER_CU
#define DGREP_MAX_WG_PER_CU 64
#endif
#ifndef DGREP_SHENG_MAPS
#define DGREP_SHENG_MAPS 1
#endif
// A/B knobs: long_dfa_seg1_kernel and verify_kernel (one 1024-thread workgroup
// per CU) read the whole-DFA LDS image (build_ximg) when the pattern has one
#ifndef DGREP_LONG_XREC
#define DGREP_LONG_XREC 1
#endif
#ifndef DGREP_VERIFY_XREC
#define DGREP_VERIFY_XREC 1
#endif
namespace dgrep {
// scan_dfa.hip
uint64_t scan_tile_bytes(int kind, uint32_t table_bytes, uint64_t n, uint64_t resident_blocks, uint32_t force,
                         double density, uint32_t spill_per_lane, uint32_t* chunk, uint32_t* waves_per_block,
                         uint32_t* slots, uint32_t* threads, bool* spills);
uint32_t scan_max_lane_chunk();
hipError_t scan_dfa_occupancy(int kind, uint32_t table_bytes, int* blocks_per_cu);
hipError_t scan_dfa(int kind, const ScanArgs& a, int grid, hipStream_t stream);
hipError_t scan_dfa_overflow(int kind, const ScanArgs& a, uint64_t nover, hipStream_t stream);
hipError_t order_lines(const TileInfo* tiles, const StagedLine* staging, uint64_t ntiles, uint64_t* out_off,
                       uint64_t* line_base, uint64_t staging_cap, uint64_t capacity, uint64_t* line_no,
                       uint64_t* start, uint64_t* len, const unsigned long long* spec, hipStream_t stream);
hipError_t verify_candidates(const VerifyArgs& v, bool candidates, hipStream_t stream);
hipError_t long_lines_end(const LongArgs& la, hipStream_t stream);
hipError_t long_lines_resolve(const LongArgs& la, hipStream_t stream);
hipError_t long_lines_sheng(const LongArgs& la, hipStream_t stream);
hipError_t long_lines_dfa(const LongDfaArgs& la, bool u32, hipStream_t stream);
uint32_t long_lookback();
uint32_t long_guesses();
}  // namespace dgrep

using namespace dgrep;

constexpr size_t kCounters = 8;
constexpr size_t kCtrLongWalk = 5;  // [5], [6]: long_dfa_fix_kernel's segments walked / re-run

// The loaded pattern's device buffers: each the upload of the PatternImage
// vector of its name (null where that is empty).
struct PatternDevice {
  uint8_t* table = nullptr;  // the stepper's image
  void* full = nullptr;
  uint8_t* cls = nullptr;    // [256] byte classes, with `full`
  uint8_t* ximg = nullptr;
  uint32_t* nfa = nullptr;
  uint8_t* long_tbl = nullptr;
  uint32_t* st2id = nullptr;
  // carry_ensure's uploads: the plain DFA; cls [256], then absorbing [nstates]
  void* carry_trans = nullptr;
  uint8_t* carry_aux = nullptr;
};

static void free_pattern_device(PatternDevice* d) {
  void* bufs[] = {d->table, d->full, d->cls, d->ximg, d->nfa, d->long_tbl, d->st2id, d->carry_trans, d->carry_aux};
  for (void* b : bufs)
    if (b) (void)hipFree(b);
  *d = PatternDevice();
}

struct dgrep_ctx {
  int device = 0;
  int num_cus = 0;
  Stream own_stream;  // before every buffer and event: destroyed after them
  hipStream_t stream = nullptr;
  std::string err;

  // loaded pattern (dgrep_load_dfa): its host side -- the vectors that were
  // uploaded dropped, h_trans and long_seed kept -- and its device buffers
  bool loaded = false;
  uint64_t load_gen = 0;  // successful loads: a stream opened under another pattern is refused (dgrep_stream_*)
  PatternImage pat;
  PatternDevice dev;
  int blocks_per_cu = 1;
  // dgrep_set_stepper: force a stepper (0 auto, 2 u8 table, 3 pair, 4 filter) /
  // cap the filter stepper's LDS rows (tests, tuning)
  int force_stepper = 0;
  uint32_t filter_rows_cap = UINT32_MAX;
  uint32_t lane_chunk = 0;  // dgrep_set_lane_chunk (0 = adaptive)

  // per-scan scratch (grown on demand, reused)
  DevBuf<TileInfo> d_tiles;
  DevBuf<uint64_t> d_out_off, d_line_base;
  DevBuf<StagedLine> d_staging;
  // device counters: [0] staging append counter, [1] overflow lanes, [2] parked
  // lines, [3] dropped candidates, [4] claimed tiles
  DevBuf<unsigned long long> d_counters;
  DevBuf<OverflowLane> d_overflow;
  DevBuf<uint2> d_spill;            // HBM spill areas of the resident threads (ScanArgs::spill)
  DevBuf<uint64_t> d_tails;         // ScanArgs::tails (resident threads x streams)
  DevBuf<uint32_t> d_chunk_nl;      // '\n' per chunk (ScanArgs::chunk_nl)
  DevBuf<ChunkMap> d_chunk_map;     // Sheng: per-chunk maps (ScanArgs::chunk_map)
  DevBuf<PendingLine> d_pend;       // parked long lines
  // long lines (dev.long_tbl / dev.st2id on the Sheng, pair and table steppers)
  DevBuf<LongSeg> d_seg;
  DevBuf<uint64_t> d_seg_off;
  DevBuf<uint8_t> d_segmap;
  // filter stepper: parked lines on the whole DFA (long_dfa_* kernels)
  DevBuf<uint64_t> d_seg_from;
  DevBuf<uint32_t> d_seg_state;  // [2][guesses][nseg]: guesses, exits

  // dgrep_scan (host data) buffers
  DevBuf<uint8_t> d_data;
  DevBuf<uint64_t> d_res_line, d_res_start, d_res_len;  // grown together (grow_results)

  Event ev0, ev1, ev2, ev3, ev4, ev5;
  uint64_t staged_hint = 0;  // kStepFilter: staged lines (candidates included) of the last scan
  float last_ms = 0.f;
  double ms_sum = 0.0;  // last_ms summed over the dgrep_scan_device calls since dgrep_take_kernel_ms
  uint64_t ms_scans = 0;
  dgrep_scan_stats stats{};
  // matching lines per byte of the last scan of the loaded pattern (0 after
  // dgrep_load_dfa): caps the adaptive lane chunk (scan_tile_bytes)
  double density = 0.0;

  // ingest (worker split -> HBM): the staging ring, its copy stream and the
  // dgrep_set_ingest settings (ingest.h)
  IngestRing ing;
  float last_ingest_ms = 0.f;

  // partition + intermediate writer (dgrep_encode_device / dgrep_map_partitions)
  DevBuf<uint8_t> d_enc_scratch, d_fname;
  DevBuf<uint64_t> d_bounds;
  DevBuf<uint8_t> d_enc_out;
  float last_encode_ms = 0.f;
  uint32_t long_value = 0;  // dgrep_set_long_value: 0 = each writer's default (kLongValueDefault, kLongValueResidentDefault)
  dgrep_encode_stats enc_stats = {};  // dgrep_last_encode_stats (encode_ms is filled in by the getter)

  // many splits in one scan (dgrep_scan_batch*, kernels/batch.h)
  DevBuf<uint64_t> d_bat_begin;             // [k + 1]
  DevBuf<unsigned long long> d_bat_lines;   // [k]
  DevBuf<unsigned long long> d_bat_sums;    // [kBatchScanBlocks] + the separator flag
  PinnedBuf<unsigned long long> h_bat_flag;  // the flag's readback rides the scan's own host wait
  std::vector<uint64_t> bat_begin;           // host copy of begin[] (read by an async upload)
  DevBuf<uint32_t> d_res_split;              // dgrep_scan_batch (host data) results, with d_res_*
  DevBuf<uint64_t> d_res_sbegin;
  Event evb0, evb1, evb2, evb3;  // made by the first batch scan
  float last_newline_ms = 0.f, last_rebase_ms = 0.f;
  // partition writer over a batch (dgrep_map_partitions_batch / dgrep_encode_batch_device)
  DevBuf<uint8_t> d_bat_names;   // the filename table: offsets [k + 1], hash states [k], escaped names
  DevBuf<uint64_t> d_bat_cells;  // [k * nreduce + 1]

  // reduce task (dgrep_reduce)
  DevBuf<uint8_t> d_red_scratch, d_red_out;
  // every reduce task of a job in one pass (dgrep_reduce_batch* / dgrep_grep_job, kernels/reduce_batch.h)
  DevBuf<uint64_t> d_rb_seg;  // the segment table [nseg + 1] of the forms that take it from the host
  DevBuf<uint64_t> d_rb_off;  // part_off [nparts + 1], then lines_in [nparts]
  Event evr0, evr1;           // made by the first batch reduce
  float last_reduce_ms = 0.f;
  // the host pack buffer of the last closed job (dgrep_job_*): the next job takes it over, touched pages and all
  uint8_t* h_job_pack = nullptr;
  size_t h_job_pack_cap = 0;

  // a bounded stream's carry walk (kernels/carry.h) over pat.h_trans: uploaded
  // to dev.carry_* the first time a stream folds, so a context that never
  // folds pays only the host bytes
  CarryTable carry;
  bool carry_ready = false;
};

namespace {

int hip_fail(dgrep_ctx* c, hipError_t e, const char* what) {
  c->err = std::string(what) + ": " + hipGetErrorString(e);
  return DGREP_E_HIP;
}
#define HIPCHK(expr)                                   \
  do {                                                 \
    hipError_t e_ = (expr);                            \
    if (e_ != hipSuccess) return hip_fail(c, e_, #expr); \
  } while (0)

// The discard-grow of a context, stream or job buffer (DevBuf::discard). The
// early-out is inline: scan_resident makes about ten of these calls per scan.
template <class T>
inline int grow(dgrep_ctx* c, DevBuf<T>& b, uint64_t need) {
  if (b.holds(need)) return DGREP_OK;
  const char* what = "";
  const hipError_t e = b.discard(need, &what);
  return e == hipSuccess ? DGREP_OK : hip_fail(c, e, what);
}

// Host wait per scan (scan_resident): block on the scan kernel's end event,
// then poll the stream for the short tail (ordering passes, the 32-B count
// copy) for at most DGREP_SYNC_SPIN_US microseconds before a blocking wait.
// The poll holds one host core per rank busy for that tail (C3: ~0.16 ms per
// scan, C2: ~0.05 ms); the blocking wait alone returned tens of µs after the
// copy (profiles/r05/ablation/sync_spin.txt). 0: always the blocking wait.
#ifndef DGREP_SYNC_SPIN_US
#define DGREP_SYNC_SPIN_US 1000
#endif

}  // namespace

extern "C" int dgrep_pick_device(int worker_id, int* device) {
  if (!device) return DGREP_E_INVALID;
  *device = -1;
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return DGREP_E_HIP;
  long dev;
  if (const char* e = getenv("DGREP_DEVICE")) {
    char* end = nullptr;
    dev = strtol(e, &end, 10);
    if (!*e || *end || dev < 0) return DGREP_E_INVALID;
    if (dev >= count) return DGREP_E_HIP;
  } else {
    long id = worker_id;
    if (id < 0) {
      const char* w = getenv("DGREP_WORKER_ID");
      char* end = nullptr;
      id = w && *w ? strtol(w, &end, 10) : -1;
      if (id < 0 || (end && *end)) id = long(getpid());
    }
    dev = id % count;
  }
  *device = int(dev);
  return DGREP_OK;
}

extern "C" int dgrep_open(int device, dgrep_ctx** out) {
  if (!out) return DGREP_E_INVALID;
  *out = nullptr;
  dgrep_ctx* c = new dgrep_ctx();
  c->device = device;
  hipError_t e = hipSetDevice(device);
  if (e == hipSuccess) e = hipDeviceGetAttribute(&c->num_cus, hipDeviceAttributeMultiprocessorCount, device);
  if (e == hipSuccess) e = c->own_stream.create();
  for (Event* ev : {&c->ev0, &c->ev1, &c->ev2, &c->ev3, &c->ev4, &c->ev5})
    if (e == hipSuccess) e = ev->create();
  const char* what = "";
  if (e == hipSuccess) e = c->d_counters.discard(kCounters, &what);
  if (e != hipSuccess) {
    // keep the context so the caller can read the message
    c->err = std::string("dgrep_open: ") + hipGetErrorString(e);
    *out = c;
    return DGREP_E_HIP;
  }
  c->stream = c->own_stream;
  *out = c;
  return DGREP_OK;
}

extern "C" void dgrep_close(dgrep_ctx* c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  free_pattern_device(&c->dev);
  if (c->ing.copy_stream) (void)hipStreamSynchronize(c->ing.copy_stream);
  free(c->h_job_pack);
  delete c;  // its members release what they hold, the streams last
}

extern "C" const char* dgrep_last_error(dgrep_ctx* c) { return c ? c->err.c_str() : "null context"; }

// for exchange.hip (the communicator runs on its context's device and stream)
namespace dgrep {
int ctx_device(const dgrep_ctx* c) { return c->device; }
hipStream_t ctx_stream(const dgrep_ctx* c) { return c->stream; }
}  // namespace dgrep

extern "C" int dgrep_set_stream(dgrep_ctx* c, void* s) {
  if (!c) return DGREP_E_INVALID;
  c->stream = s ? static_cast<hipStream_t>(s) : c->own_stream;
  return DGREP_OK;
}

extern "C" int dgrep_set_lane_chunk(dgrep_ctx* c, uint32_t chunk_bytes) {
  if (!c) return DGREP_E_INVALID;
  if (chunk_bytes && (chunk_bytes % 128 || chunk_bytes < 4096 || chunk_bytes > scan_max_lane_chunk())) {
    c->err = "lane chunk must be 0 or a multiple of 128 in [4096, " + std::to_string(scan_max_lane_chunk()) + "]";
    return DGREP_E_INVALID;
  }
  c->lane_chunk = chunk_bytes;
  return DGREP_OK;
}

extern "C" int dgrep_set_long_value(dgrep_ctx* c, uint32_t bytes) {
  if (!c) return DGREP_E_INVALID;
  if (bytes && (bytes % 64 || bytes < 256 || bytes > (1u << 30))) {
    c->err = "long value must be 0 or a multiple of 64 in [256, 2^30]";
    return DGREP_E_INVALID;
  }
  c->long_value = bytes;
  return DGREP_OK;
}

extern "C" int dgrep_set_stepper(dgrep_ctx* c, int force, uint32_t filter_rows) {
  // 1 (the r01 wide stepper) and 5 (the r05 word stepper) were removed in round 6
  if (!c || force < 0 || force > 4 || force == 1) return DGREP_E_INVALID;
  c->force_stepper = force;
  c->filter_rows_cap = filter_rows ? filter_rows : UINT32_MAX;
  return DGREP_OK;
}

// vector -> a fresh device allocation (a multiple of 16 bytes); an empty vector leaves *p null
template <class P, class V>
static hipError_t upload(const std::vector<V>& v, P** p) {
  if (v.empty()) return hipSuccess;
  const size_t bytes = v.size() * sizeof(V);
  const hipError_t e = hipMalloc(reinterpret_cast<void**>(p), (bytes + 15) & ~size_t(15));
  return e != hipSuccess ? e : hipMemcpy(*p, v.data(), bytes, hipMemcpyHostToDevice);
}

// build (host only, pattern_image.h) -> upload into fresh allocations -> commit:
// until the last step the context holds the previous pattern, whole (dgrep.h)
extern "C" int dgrep_load_dfa(dgrep_ctx* c, const void* blob, size_t n) {
  if (!c) return DGREP_E_INVALID;
  PatternImage img;
  std::string err;
  const int rc = build_pattern_image(blob, n, c->force_stepper, c->filter_rows_cap, &img, &err);
  if (rc != DGREP_OK) {
    c->err = err;
    return rc;
  }
  PatternDevice d;
  int bpc = 0;
  hipError_t e = hipSetDevice(c->device);
  if (e == hipSuccess) e = upload(img.table, &d.table);
  if (e == hipSuccess) e = upload(img.full, &d.full);
  if (e == hipSuccess && !img.full.empty()) e = upload(std::vector<uint8_t>(img.h_cls, img.h_cls + 256), &d.cls);
  if (e == hipSuccess) e = upload(img.ximg, &d.ximg);
  if (e == hipSuccess) e = upload(img.nfa, &d.nfa);
  if (e == hipSuccess) e = upload(img.long_tbl, &d.long_tbl);
  if (e == hipSuccess) e = upload(img.st2id, &d.st2id);
  if (e == hipSuccess) e = scan_dfa_occupancy(launch_kind(img), img.table_bytes, &bpc);
  if (e != hipSuccess) {
    free_pattern_device(&d);
    return hip_fail(c, e, "dgrep_load_dfa: upload");
  }
  free_pattern_device(&c->dev);  // the previous pattern goes now, its carry tables with it
  c->dev = d;
  c->pat = std::move(img);
  c->pat.drop_uploaded();
  c->blocks_per_cu = std::max(1, std::min(bpc, DGREP_MAX_WG_PER_CU));
  ++c->load_gen;
  c->carry_ready = false;
  c->density = 0.0;
  c->staged_hint = 0;
  c->loaded = true;
  return DGREP_OK;
}

// The lines the scan parked (npend > 0): their ends, then their segments'
// maps, then each line's verdict and length (long_* kernels in scan_dfa.hip).
// The segment cut is made on the host from the ends (one small readback).
static int resolve_long_lines(dgrep_ctx* c, const uint8_t* d_data, uint64_t n, uint64_t chunk, uint64_t nchunks,
                              uint64_t npend) {
  int rc;
  LongArgs la;
  memset(&la, 0, sizeof la);
  la.data = d_data;
  la.n = n;
  la.chunk = chunk;
  la.nchunks = nchunks;
  la.chunk_nl = c->d_chunk_nl;
  la.pend = c->d_pend;
  la.npend = npend;
  la.st2id = c->dev.st2id;
  la.tbl = c->dev.long_tbl;
  la.nstates = c->pat.long_states;
  la.start_m = c->pat.long_start_m;
  HIPCHK(long_lines_end(la, c->stream));
  std::vector<PendingLine> P(npend);
  HIPCHK(hipMemcpyAsync(P.data(), c->d_pend, npend * sizeof(PendingLine), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  // segments of about 1/4096 of the parked bytes (so the GPU fills), at least
  // 256 KiB (a wave's 64 pieces of 4 KiB) and 64-B aligned
  uint64_t total = 0;
  for (const PendingLine& p : P) total += p.end > p.resume ? p.end - p.resume : 0;
  uint64_t seg = std::max<uint64_t>(uint64_t(256) << 10, (total / 4096 + 63) & ~uint64_t(63));
  std::vector<LongSeg> segs;
  std::vector<uint64_t> off(npend + 1, 0);
  for (uint64_t i = 0; i < npend; ++i) {
    for (uint64_t b = P[i].resume; b < P[i].end; b += seg) segs.push_back(LongSeg{b, std::min(P[i].end, b + seg)});
    off[i + 1] = segs.size();
  }
  if ((rc = grow(c, c->d_seg, std::max<uint64_t>(segs.size(), 1))) != DGREP_OK) return rc;
  if ((rc = grow(c, c->d_seg_off, npend + 1)) != DGREP_OK) return rc;
  if ((rc = grow(c, c->d_segmap, std::max<uint64_t>(segs.size(), 1) * 256)) != DGREP_OK) return rc;
  if (!segs.empty())
    HIPCHK(hipMemcpyAsync(c->d_seg, segs.data(), segs.size() * sizeof(LongSeg), hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(c->d_seg_off, off.data(), off.size() * 8, hipMemcpyHostToDevice, c->stream));
  la.seg = c->d_seg;
  la.nseg = segs.size();
  la.seg_off = c->d_seg_off;
  la.segmap = c->d_segmap;
  HIPCHK(long_lines_resolve(la, c->stream));
  // the host vectors are read by the async copies above: wait before they go
  HIPCHK(hipStreamSynchronize(c->stream));
  return DGREP_OK;
}

// The filter stepper's parked lines (> 256 states): their ends from the chunk
// '\n' counts, then each line decided on the whole DFA from its start, in
// segments run in parallel from guessed entry states and checked in order
// (long_dfa_* kernels in scan_dfa.hip). Segments sized so that every resident
// lane gets about four (two at a time, stepped in lockstep), >= 16 KiB.
static int resolve_long_filter(dgrep_ctx* c, const uint8_t* d_data, uint64_t n, uint64_t chunk, uint64_t nchunks,
                               uint64_t npend) {
  int rc;
  LongArgs le;
  memset(&le, 0, sizeof le);
  le.data = d_data;
  le.n = n;
  le.chunk = chunk;
  le.nchunks = nchunks;
  le.chunk_nl = c->d_chunk_nl;
  le.pend = c->d_pend;
  le.npend = npend;
  HIPCHK(long_lines_end(le, c->stream));
  std::vector<PendingLine> P(npend);
  HIPCHK(hipMemcpyAsync(P.data(), c->d_pend, npend * sizeof(PendingLine), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  uint64_t total = 0;
  for (const PendingLine& p : P) total += p.end - p.line_start;
  // one segment per lane of ONE round of long_dfa_seg1_kernel (one
  // 1024-thread workgroup per CU): a second, partly filled round held half the
  // CUs idle for a whole segment (long_c4: 384 workgroups over 256 CUs). Each
  // line adds at most one partial segment, hence the npend in the divisor.
  // >= 16 KiB.
  const uint64_t lanes2 = uint64_t(c->num_cus) * 1024;
  const uint64_t div = npend < lanes2 / 2 ? lanes2 - npend : uint64_t(c->num_cus) * 1536;
  const uint64_t seg = std::max<uint64_t>(uint64_t(16) << 10, (total / div + 16) & ~uint64_t(15));
  std::vector<LongSeg> segs;
  std::vector<uint64_t> from, off(npend + 1, 0);
  const uint64_t lb = long_lookback();
  for (uint64_t i = 0; i < npend; ++i) {
    for (uint64_t b = P[i].line_start; b < P[i].end; b += seg) {
      segs.push_back(LongSeg{b, std::min(P[i].end, b + seg)});
      from.push_back(b - std::min(lb, b - P[i].line_start));
    }
    off[i + 1] = segs.size();
  }
  const uint64_t ns = std::max<uint64_t>(segs.size(), 1);
  if ((rc = grow(c, c->d_seg, ns)) != DGREP_OK) return rc;
  if ((rc = grow(c, c->d_seg_from, ns)) != DGREP_OK) return rc;
  const uint64_t ng = long_guesses();
  if ((rc = grow(c, c->d_seg_state, 2 * ng * ns)) != DGREP_OK) return rc;
  if ((rc = grow(c, c->d_seg_off, npend + 1)) != DGREP_OK) return rc;
  if (!segs.empty()) {
    HIPCHK(hipMemcpyAsync(c->d_seg, segs.data(), segs.size() * sizeof(LongSeg), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(c->d_seg_from, from.data(), from.size() * 8, hipMemcpyHostToDevice, c->stream));
  }
  HIPCHK(hipMemcpyAsync(c->d_seg_off, off.data(), off.size() * 8, hipMemcpyHostToDevice, c->stream));
  LongDfaArgs la;
  memset(&la, 0, sizeof la);
  la.data = d_data;
  la.full = c->dev.full;
  la.hot_entries = c->pat.verify_hot;
  {
    const size_t esz = c->pat.full_u32 ? 4 : 2, ne = size_t(c->pat.nstates) * c->pat.nclasses;
    la.seg_hot_entries = uint32_t(std::min<size_t>(ne, kLongDfaHotBytes / esz)) / c->pat.nclasses * c->pat.nclasses;
  }
  la.nclasses = c->pat.nclasses;
  la.cls = c->dev.cls;
  la.start = c->pat.blob_start;
  la.start_m = c->pat.blob_start_m;
  la.matched = c->pat.blob_matched;
  la.dead = c->pat.blob_dead;
  for (uint32_t i = 0; i < uint32_t(kLongSeeds); ++i) la.seed[i] = c->pat.long_seed[i];
  la.seg = c->d_seg;
  la.seg_from = c->d_seg_from;
  la.nseg = segs.size();
  la.seg_guess = c->d_seg_state;
  la.seg_exit = c->d_seg_state + ng * ns;
  la.seg_off = c->d_seg_off;
  la.pend = c->d_pend;
  la.npend = npend;
  la.ximg = DGREP_LONG_XREC ? c->dev.ximg : nullptr;
  la.ximg_bytes = c->pat.ximg_bytes;
  la.x_hot = c->pat.x_hot;
  la.xr_off = c->pat.xr_off;
  // the fix kernel's tallies: two of the scan's counters, zeroed before the scan
  la.walk_count = c->d_counters + kCtrLongWalk;
  HIPCHK(long_lines_dfa(la, c->pat.full_u32, c->stream));
  unsigned long long walk[2] = {0, 0};
  HIPCHK(hipMemcpyAsync(walk, la.walk_count, sizeof walk, hipMemcpyDeviceToHost, c->stream));
  // the host vectors are read by the async copies above: wait before they go
  HIPCHK(hipStreamSynchronize(c->stream));
  c->stats.long_segments = uint32_t(std::min<unsigned long long>(walk[0], UINT32_MAX));
  c->stats.long_guess_misses = uint32_t(std::min<unsigned long long>(walk[1], UINT32_MAX));
  return DGREP_OK;
}

// long_lines_sheng's arguments: the Sheng stepper's parked lines, resolved
// through the chunk maps
static LongArgs sheng_long_args(dgrep_ctx* c, const uint8_t* d_data, uint64_t n, uint64_t chunk, uint64_t nchunks,
                                uint64_t npend) {
  LongArgs la;
  memset(&la, 0, sizeof la);
  la.n = n;
  la.chunk = chunk;
  la.nchunks = nchunks;
  la.pend = c->d_pend;
  la.npend = npend;
  la.chunk_map = c->d_chunk_map;
  la.sheng_m = c->pat.start_m;
  la.nl_lo = c->pat.sheng_nl_lo;
  la.nl_hi = c->pat.sheng_nl_hi;
  la.sheng_v = reinterpret_cast<const uint2*>(c->dev.table);
  la.data = d_data;
  return la;
}

// Core of every scan: the split is resident at d_data (n bytes). Results go to
// device arrays of `capacity` lines; *count receives the number of matches.
static int scan_resident(dgrep_ctx* c, const uint8_t* d_data, uint64_t n, uint64_t* d_line, uint64_t* d_start,
                         uint64_t* d_len, uint64_t capacity, uint64_t* count) {
  *count = 0;
  dgrep_scan_stats& S = c->stats;
  S = dgrep_scan_stats{};
  S.stepper = uint32_t(c->pat.step_kind);
  c->last_ms = 0.f;
  if (c->pat.flags & DGREP_DFA_MATCH_NONE) return DGREP_OK;
  if (n == 0) {
    // strings.Split("", "\n") == [""]: one empty line, line 1
    if (!c->pat.empty_line_matches) return DGREP_OK;
    *count = 1;
    S.matches = 1;
    if (capacity >= 1) {
      const uint64_t one = 1, zero = 0;
      HIPCHK(hipMemcpyAsync(d_line, &one, 8, hipMemcpyHostToDevice, c->stream));
      HIPCHK(hipMemcpyAsync(d_start, &zero, 8, hipMemcpyHostToDevice, c->stream));
      HIPCHK(hipMemcpyAsync(d_len, &zero, 8, hipMemcpyHostToDevice, c->stream));
      HIPCHK(hipStreamSynchronize(c->stream));
    }
    return DGREP_OK;
  }
  if (reinterpret_cast<uintptr_t>(d_data) & 15) {
    c->err = "device split must be 16-byte aligned";
    return DGREP_E_INVALID;
  }
  const uint64_t resident = uint64_t(c->num_cus) * uint64_t(c->blocks_per_cu);
  uint32_t chunk = 0, wpb = 1, slots = 0, threads = 0;
  bool spills = false;
  const uint64_t tile = scan_tile_bytes(launch_kind(c->pat), c->pat.table_bytes, n, resident, c->lane_chunk, c->density,
                                        DGREP_SPILL_RECORDS, &chunk, &wpb, &slots, &threads, &spills);
  const uint64_t ntiles = (n + tile - 1) / tile;
  int rc;
  if ((rc = grow(c, c->d_tiles, ntiles)) != DGREP_OK) return rc;
  if ((rc = grow(c, c->d_out_off, ntiles + 1)) != DGREP_OK) return rc;
  if ((rc = grow(c, c->d_line_base, ntiles + 1)) != DGREP_OK) return rc;
  // kStepFilter stages its candidates too: the staging buffer holds at least
  // the previous scan's staged lines, and grows (one re-scan) if they overflow
  const bool filt = c->pat.step_kind == kStepFilter && c->pat.cand_end != UINT32_MAX;
  if ((rc = grow(c, c->d_staging, filt ? std::max(capacity, c->staged_hint) : capacity)) != DGREP_OK)
    return rc;

  if (!c->d_overflow && (rc = grow(c, c->d_overflow, 1u << 16)) != DGREP_OK) return rc;
  const int grid = int(std::min<uint64_t>(ntiles, resident));
  // chunks per lane (the two-stream steppers step two in lockstep)
  const uint32_t streams = tile / (uint64_t(kTileLanes) * chunk);
  const bool use_spill = spills && DGREP_SPILL_RECORDS > 0;
  if (use_spill && (rc = grow(c, c->d_spill, uint64_t(grid) * threads * streams * DGREP_SPILL_RECORDS)) != DGREP_OK)
    return rc;
  // long lines: the lanes' tail entries, '\n' per chunk and the pending list
  // (parking needs the blob's table: <= 256-state DFAs on the Sheng / pair /
  // table steppers)
  if ((rc = grow(c, c->d_tails, uint64_t(grid) * threads * streams)) != DGREP_OK) return rc;
  // the filter parks too when the whole DFA is at hand (not a partial blob, whose
  // candidates an NFA program decides: its lanes read a long line on)
  const bool park_filter = DGREP_PARK && c->pat.step_kind == kStepFilter && c->dev.full != nullptr;
  const bool park = (DGREP_PARK && c->dev.long_tbl != nullptr) || park_filter;
  const uint64_t nchunks = (n + chunk - 1) / chunk;
  // Sheng: the chunk maps replace the '\n' counts (long_sheng_kernel)
  const bool park_maps = park && c->pat.step_kind == kStepSheng8 && DGREP_SHENG_MAPS;
  if (park) {
    if (park_maps) {
      if ((rc = grow(c, c->d_chunk_map, nchunks)) != DGREP_OK) return rc;
    } else if ((rc = grow(c, c->d_chunk_nl, nchunks)) != DGREP_OK) {
      return rc;
    }
    if (!c->d_pend && (rc = grow(c, c->d_pend, 1024)) != DGREP_OK) return rc;
  }

  ScanArgs a;
  memset(&a, 0, sizeof a);
  a.data = d_data;
  a.n = n;
  a.table = c->dev.table;
  a.table_bytes = c->pat.table_bytes;
  a.start = c->pat.start;
  a.start_m = c->pat.start_m;
  a.chunk = chunk;
  a.ntiles = ntiles;
  a.counter = c->d_counters;
  a.tiles = c->d_tiles;
  a.overflow_count = c->d_counters + 1;
  a.pend_count = c->d_counters + 2;
  a.tile_next = c->d_counters + 4;
  a.tails = c->d_tails;
  a.chunk_nl = park && !park_maps ? c->d_chunk_nl : nullptr;
  a.chunk_map = park_maps ? c->d_chunk_map : nullptr;
  a.nclasses = c->pat.nclasses;
  a.pair_t1 = c->pat.pair_args.t1;
  a.pair_thr = c->pat.pair_args.thr;
  a.pair_div = c->pat.pair_args.div;
  a.cand_end = c->pat.cand_end;
  a.spill = use_spill ? c->d_spill : nullptr;
  a.spill_per_lane = use_spill ? DGREP_SPILL_RECORDS : 0;
  // every resident workgroup is launched even when the last round of tiles is
  // part-empty: trimming the grid so that every wave runs the same number of
  // tiles leaves some CUs with 2 workgroups and others with 3, and the time
  // follows the fullest CU (C2 16 KiB chunks: 4.13 TB/s trimmed, 4.74 full)
  (void)wpb;
  unsigned long long ctr[4] = {0, 0, 0, 0};
  S.lane_chunk = chunk;
  S.lane_slots = slots;
  S.tiles = ntiles;
  // The common case -- no overflowing lane, no parked line, no filter
  // candidates -- takes ONE host synchronisation per scan: the ordering passes
  // are queued right behind the scan (they read the tiles' counts on the device
  // and never write past `capacity`) and the counters are read back after them.
  // Anything else shows in the counters, and the ordering is queued again once
  // the extra passes have run.
  const bool speculate = !filt && capacity != 0;
  // Each buffer a scan can outgrow (overflow list, pending list, the filter's
  // staging) is grown to what the scan counted and the scan re-run, so every
  // grow is followed by a scan that fits: at most three grows, four scans. (A
  // loop that could end on a grow left the filter's candidates unverified but
  // counted.)
  bool settled = false;
  for (int attempt = 0; attempt < 4 && !settled; ++attempt) {
    a.staging = c->d_staging;
    a.capacity = c->d_staging.cap;
    a.overflow = c->d_overflow;
    a.overflow_cap = c->d_overflow.cap;
    a.pend = park ? c->d_pend : nullptr;
    a.pend_cap = park ? c->d_pend.cap : 0;
    HIPCHK(hipMemsetAsync(c->d_counters, 0, kCounters * sizeof(unsigned long long), c->stream));
    HIPCHK(hipEventRecord(c->ev0, c->stream));
    HIPCHK(scan_dfa(launch_kind(c->pat), a, grid, c->stream));
    HIPCHK(hipEventRecord(c->ev1, c->stream));
    // (the kernel reads the counters itself and leaves the arrays alone if a
    // lane overflowed or a line was parked: entries [count, capacity) are never
    // written, and a parked line that does not match would be one)
    if (speculate)
      HIPCHK(order_lines(c->d_tiles, c->d_staging, ntiles, c->d_out_off, c->d_line_base, c->d_staging.cap, capacity,
                         d_line, d_start, d_len, c->d_counters, c->stream));
    HIPCHK(hipMemcpyAsync(ctr, c->d_counters, sizeof ctr, hipMemcpyDeviceToHost, c->stream));
    if (DGREP_SYNC_SPIN_US > 0) {
      // block until the scan kernel is done (its wake-up latency overlaps the
      // ordering passes), then poll the short tail, bounded (see DGREP_SYNC_SPIN_US)
      HIPCHK(hipEventSynchronize(c->ev1));
      const auto t0 = std::chrono::steady_clock::now();
      hipError_t q;
      while ((q = hipStreamQuery(c->stream)) == hipErrorNotReady &&
             std::chrono::steady_clock::now() - t0 < std::chrono::microseconds(DGREP_SYNC_SPIN_US)) {
      }
      if (q == hipErrorNotReady) q = hipStreamSynchronize(c->stream);
      HIPCHK(q);
    } else {
      HIPCHK(hipStreamSynchronize(c->stream));
    }
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, c->ev0, c->ev1));
    S.scan_ms += ms;  // a re-run scan is counted: it is part of this call's device time
    ++S.scan_attempts;
    if (ctr[1] > c->d_overflow.cap) {
      // more overflowing lanes than recorded: grow the list and scan again
      if ((rc = grow(c, c->d_overflow, ctr[1])) != DGREP_OK) return rc;
    } else if (park && ctr[2] > c->d_pend.cap) {
      // more parked long lines than the pending list holds
      if ((rc = grow(c, c->d_pend, ctr[2])) != DGREP_OK) return rc;
    } else if (filt && ctr[0] > c->d_staging.cap) {
      // candidates included, more staged lines than the staging buffer holds
      if ((rc = grow(c, c->d_staging, ctr[0] + ctr[0] / 8)) != DGREP_OK) return rc;
    } else if (park && ctr[2] && ctr[0] > c->d_staging.cap && capacity != 0 && ctr[0] - ctr[2] <= capacity) {
      // every parked line is staged as one record whether it matches or not: the
      // staged lines outgrew the staging buffer (sized by `capacity`), but the
      // matching ones may still fit the caller's arrays once the parked lines
      // that do not match are dropped -- and only complete staging can be
      // resolved and ordered. (Ordering the truncated staging here returned a
      // count <= capacity with wrong records.)
      if ((rc = grow(c, c->d_staging, ctr[0])) != DGREP_OK) return rc;
    } else {
      settled = true;
    }
  }
  if (!settled) {
    c->err = "scan buffers still too small after three grows";
    return DGREP_E_HIP;
  }
  const uint64_t staged = ctr[0];
  const uint64_t npend = park ? ctr[2] : 0;
  S.overflow_lanes = ctr[1];
  S.pending = npend;
  c->last_ms = S.scan_ms;
  // matching (and candidate) lines per byte: caps the next scan's lane chunk
  c->density = double(staged) / double(n);
  const bool over = ctr[1] && staged <= a.capacity;
  if (over) {
    HIPCHK(hipEventRecord(c->ev2, c->stream));
    HIPCHK(scan_dfa_overflow(launch_kind(c->pat), a, ctr[1], c->stream));
    HIPCHK(hipEventRecord(c->ev3, c->stream));
  }
  uint64_t total = staged;
  // verification pass: the filter's candidates, parked long lines
  const bool verify = filt || npend;
  bool ordered = false;  // the verification branch queued the ordering already
  if (verify && staged && staged <= a.capacity) {
    VerifyArgs v;
    memset(&v, 0, sizeof v);
    v.data = d_data;
    v.full = c->dev.full;
    v.full_u32 = c->pat.full_u32 ? 1u : 0u;
    v.hot_entries = c->pat.verify_hot;
    v.cls = c->dev.cls;
    v.nclasses = c->pat.nclasses;
    v.start = c->pat.blob_start;
    v.start_m = c->pat.blob_start_m;
    v.tiles = c->d_tiles;
    v.ntiles = ntiles;
    v.staging = c->d_staging;
    v.staging_cap = c->d_staging.cap;
    v.removed = c->d_counters + 3;  // zeroed before the scan
    v.nfa = c->dev.nfa;
    v.nfa_words = c->pat.nfa_words;
    v.matched = c->dev.nfa ? UINT32_MAX : c->pat.blob_matched;
    v.pend = c->d_pend;
    v.ximg = DGREP_VERIFY_XREC ? c->dev.ximg : nullptr;
    v.ximg_bytes = c->pat.ximg_bytes;
    v.x_hot = c->pat.x_hot;
    v.xr_off = c->pat.xr_off;
    v.num_cus = uint32_t(c->num_cus);
    HIPCHK(hipEventRecord(c->ev4, c->stream));
    if (npend && park_maps) {
      HIPCHK(long_lines_sheng(sheng_long_args(c, d_data, n, chunk, nchunks, npend), c->stream));
    } else if (npend && park_filter) {
      if ((rc = resolve_long_filter(c, d_data, n, chunk, nchunks, npend)) != DGREP_OK) return rc;
    } else if (npend && (rc = resolve_long_lines(c, d_data, n, chunk, nchunks, npend)) != DGREP_OK) {
      return rc;
    }
    HIPCHK(verify_candidates(v, filt, c->stream));
    HIPCHK(hipEventRecord(c->ev5, c->stream));
    unsigned long long removed = 0;
    HIPCHK(hipMemcpyAsync(&removed, c->d_counters + 3, 8, hipMemcpyDeviceToHost, c->stream));
    // nothing changes the staged lines after the verification: when every
    // staged line fits the output, order them before the one host wait (the
    // kept lines are fewer still; a separate wait cost C4 ~30 us a scan)
    if (capacity != 0 && staged <= capacity) {
      HIPCHK(order_lines(c->d_tiles, c->d_staging, ntiles, c->d_out_off, c->d_line_base, c->d_staging.cap, capacity,
                         d_line, d_start, d_len, nullptr, c->stream));
      ordered = true;
    }
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipEventElapsedTime(&S.verify_ms, c->ev4, c->ev5));
    c->last_ms += S.verify_ms;
    total = staged - removed;
    S.candidates = removed;  // dropped ones; kept candidates count as matches
  } else if (npend && staged > a.capacity) {
    // The staged lines did not fit (a size query, or too small a capacity), so
    // no record is resolved -- but the count must still be exact: every parked
    // line was counted as one staged record, so resolve the pending list (it
    // does not depend on staging) and subtract the parked lines that do not
    // match. (Overflow lanes were counted in full by the scan: no pass needed.)
    HIPCHK(hipEventRecord(c->ev4, c->stream));
    if (park_maps) {
      HIPCHK(long_lines_sheng(sheng_long_args(c, d_data, n, chunk, nchunks, npend), c->stream));
    } else if ((rc = park_filter ? resolve_long_filter(c, d_data, n, chunk, nchunks, npend)
                                 : resolve_long_lines(c, d_data, n, chunk, nchunks, npend)) != DGREP_OK) {
      return rc;
    }
    HIPCHK(hipEventRecord(c->ev5, c->stream));
    std::vector<PendingLine> P(npend);
    HIPCHK(hipMemcpyAsync(P.data(), c->d_pend, npend * sizeof(PendingLine), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipEventElapsedTime(&S.verify_ms, c->ev4, c->ev5));
    c->last_ms += S.verify_ms;
    uint64_t unmatched = 0;
    for (const PendingLine& p : P) unmatched += p.matched ? 0u : 1u;
    total = staged - unmatched;
  }
  if (filt) c->staged_hint = staged;
  S.matches = total;
  *count = total;
  // the speculative ordering stands (and ran: the kernel tests the same two
  // counters) unless a lane overflowed or a line was parked
  const bool spec_stands = speculate && !ctr[1] && !ctr[2];
  const bool order = total != 0 && total <= capacity && !spec_stands && !ordered;
  if (order)
    HIPCHK(order_lines(c->d_tiles, c->d_staging, ntiles, c->d_out_off, c->d_line_base, c->d_staging.cap, capacity,
                       d_line, d_start, d_len, nullptr, c->stream));
  if (over || order) HIPCHK(hipStreamSynchronize(c->stream));
  if (over) {
    HIPCHK(hipEventElapsedTime(&S.overflow_ms, c->ev2, c->ev3));
    c->last_ms += S.overflow_ms;
  }
  return DGREP_OK;
}

extern "C" int dgrep_scan_device(dgrep_ctx* c, const void* d_data, size_t n, uint64_t* d_line_no, uint64_t* d_start,
                                 uint64_t* d_len, uint64_t capacity, uint64_t* count) {
  if (!c || !count || (n && !d_data)) return DGREP_E_INVALID;
  if (!c->loaded) { c->err = "no DFA loaded"; return DGREP_E_NO_DFA; }
  HIPCHK(hipSetDevice(c->device));
  const int rc = scan_resident(c, static_cast<const uint8_t*>(d_data), n, d_line_no, d_start, d_len, capacity, count);
  if (rc == DGREP_OK) {
    c->ms_sum += c->last_ms;
    ++c->ms_scans;
  }
  return rc;
}

// a failed call of ingest.h, as HIPCHK reports one
#define INGCHK(expr)                                             \
  do {                                                           \
    hipError_t e_ = (expr);                                      \
    if (e_ != hipSuccess) return hip_fail(c, e_, c->ing.what);   \
  } while (0)

// Worker-side ingest (the bytes map_reduce/worker.go:72-76 read with
// os.ReadFile and hand to Map) with the resident completion contract: P (k
// buffers, `total` bytes, ingest.h) -> c->d_data. On the ring path the first
// DMA waits for earlier work on the context stream (the previous scan may still
// read d_data), the context stream is ordered behind the last DMA and the copy
// stream is drained: the caller's bytes are free on return. The direct path is
// one copy on the context stream.
static int ingest_resident(dgrep_ctx* c, const uint8_t* const* data, const size_t* n, size_t k, size_t total,
                           bool sep = true) {
  const auto t0 = std::chrono::steady_clock::now();
  IngestRing* r = &c->ing;
  if (ingest_direct(*r, total)) {
    INGCHK(ingest_direct_copy(r, data, n, k, sep, c->d_data, total, c->stream));
    c->last_ingest_ms = 0.f;
    return DGREP_OK;
  }
  INGCHK(ingest_ring(r));
  HIPCHK(hipEventRecord(c->ev1, c->stream));
  HIPCHK(hipStreamWaitEvent(r->copy_stream, c->ev1, 0));
  INGCHK(ingest_pieces(r, data, n, k, sep, c->d_data, total));
  HIPCHK(hipStreamWaitEvent(c->stream, r->ev_stage[r->last], 0));
  HIPCHK(hipStreamSynchronize(r->copy_stream));
  c->last_ingest_ms =
      std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return DGREP_OK;
}

extern "C" int dgrep_set_ingest(dgrep_ctx* c, size_t chunk_bytes, int nbufs, int threads) {
  if (!c || nbufs < 0 || threads < 0 || nbufs > 64 || threads > 256) return DGREP_E_INVALID;
  c->ing.chunk = chunk_bytes;
  if (nbufs) c->ing.bufs = nbufs;
  if (threads) c->ing.threads = threads;
  return DGREP_OK;
}

extern "C" int dgrep_last_ingest_ms(dgrep_ctx* c, float* ms) {
  if (!c || !ms) return DGREP_E_INVALID;
  *ms = c->last_ingest_ms;
  return DGREP_OK;
}

// The context's result arrays, at least `want` lines each.
static int grow_results(dgrep_ctx* c, uint64_t want) {
  int rc;
  if ((rc = grow(c, c->d_res_line, want)) != DGREP_OK) return rc;
  if ((rc = grow(c, c->d_res_start, want)) != DGREP_OK) return rc;
  return grow(c, c->d_res_len, want);
}

// One array of a result fetch: *host = malloc(lead + bytes) (nothing when that
// is 0), and `bytes` from dev copied in behind the lead.
struct Fetch {
  void* host;  // T**
  const void* dev;
  size_t bytes, lead;
};

// Device results to malloc'd host arrays: every allocation first, and with one
// missing DGREP_E_NOMEM (the caller frees its struct); then the copies on the
// context stream and one synchronise.
static int fetch_results(dgrep_ctx* c, std::initializer_list<Fetch> arrays) {
  bool ok = true, copies = false;
  for (const Fetch& f : arrays)
    if (f.lead + f.bytes) ok = (*static_cast<void**>(f.host) = malloc(f.lead + f.bytes)) != nullptr && ok;
  if (!ok) return DGREP_E_NOMEM;
  for (const Fetch& f : arrays) {
    if (!f.bytes) continue;
    HIPCHK(hipMemcpyAsync(*static_cast<uint8_t**>(f.host) + f.lead, f.dev, f.bytes, hipMemcpyDeviceToHost, c->stream));
    copies = true;
  }
  if (copies) HIPCHK(hipStreamSynchronize(c->stream));
  return DGREP_OK;
}

// Host split -> HBM (ingest) -> scan into the context's result arrays.
static int scan_host(dgrep_ctx* c, const uint8_t* data, size_t n, uint64_t* count) {
  int rc;
  if (n) {
    if ((rc = grow(c, c->d_data, (n + 63) & ~uint64_t(63))) != DGREP_OK) return rc;
    if ((rc = ingest_resident(c, &data, &n, 1, n)) != DGREP_OK) return rc;
  }
  uint64_t want = std::max<uint64_t>(c->d_res_line.cap, std::max<uint64_t>(1024, n / 512));
  for (int attempt = 0; attempt < 2; ++attempt) {
    if ((rc = grow_results(c, want)) != DGREP_OK) return rc;
    if ((rc = scan_resident(c, c->d_data, n, c->d_res_line, c->d_res_start, c->d_res_len, c->d_res_line.cap, count)) !=
        DGREP_OK)
      return rc;
    if (*count <= c->d_res_line.cap) break;
    want = *count;
  }
  return DGREP_OK;
}

extern "C" int dgrep_scan(dgrep_ctx* c, const uint8_t* data, size_t n, dgrep_result* out) {
  if (!c || !out || (n && !data)) return DGREP_E_INVALID;
  memset(out, 0, sizeof *out);
  if (!c->loaded) { c->err = "no DFA loaded"; return DGREP_E_NO_DFA; }
  HIPCHK(hipSetDevice(c->device));
  uint64_t count = 0;
  int rc;
  if ((rc = scan_host(c, data, n, &count)) != DGREP_OK) return rc;
  out->count = count;
  if (count == 0) return DGREP_OK;
  const size_t b = count * 8;
  rc = fetch_results(c, {{&out->line_no, c->d_res_line, b, 0}, {&out->start, c->d_res_start, b, 0},
                         {&out->len, c->d_res_len, b, 0}});
  if (rc == DGREP_E_NOMEM) dgrep_result_free(out);
  return rc;
}

// ---- many splits in one scan (kernels/batch.h) ------------------------------
// One map task per input file (map_reduce/coordinator.go:312,329-333) makes a
// worker's files many small splits. Packed with one '\n' between them they
// split into exactly the splits' lines, so one scan_resident over the packed
// buffer finds every matching line; the batch kernels rebase the records.

// The batch scratch for k splits, and begin[] (c->bat_begin, k + 1 entries).
static int batch_setup(dgrep_ctx* c, const uint64_t* len, uint64_t k) {
  int rc;
  if ((rc = grow(c, c->d_bat_begin, k + 1)) != DGREP_OK) return rc;
  if ((rc = grow(c, c->d_bat_lines, k)) != DGREP_OK) return rc;
  if ((rc = grow(c, c->d_bat_sums, kBatchScanBlocks + 1)) != DGREP_OK) return rc;
  HIPCHK(c->h_bat_flag.alloc(1));
  for (Event* e : {&c->evb0, &c->evb1, &c->evb2, &c->evb3}) HIPCHK(e->create());
  c->bat_begin.resize(k + 1);
  uint64_t b = 0;
  for (uint64_t i = 0; i < k; ++i) {
    c->bat_begin[i] = b;
    b += len[i] + 1;
  }
  c->bat_begin[k] = b;  // n_packed + 1: closes the last region
  return DGREP_OK;
}

// Core of both batch forms: P (n bytes, k splits, begin[] in c->bat_begin) is
// resident at d_packed. `prepass`: count the lines before each split and check
// the separators first -- once per P; a re-scan into larger arrays reuses them.
// The kernels are queued on the context stream around scan_resident's own
// work; the separator flag's readback is queued before the scan, so the scan's
// host wait delivers it, and the one wait added is the one after the rebase.
static int batch_resident(dgrep_ctx* c, const uint8_t* d_packed, uint64_t n, uint64_t k, uint64_t* d_line,
                          uint64_t* d_start, uint64_t* d_len, uint32_t* d_split, uint64_t* d_split_begin,
                          uint64_t capacity, uint64_t* count, bool prepass) {
  *count = 0;
  BatchArgs b;
  b.data = d_packed;
  b.n = n;
  b.begin = c->d_bat_begin;
  b.k = k;
  b.lines = c->d_bat_lines;
  b.block_sums = c->d_bat_sums;
  b.bad_split = c->d_bat_sums + kBatchScanBlocks;
  if (prepass) {
    if (n && (reinterpret_cast<uintptr_t>(d_packed) & 15)) {
      c->err = "device split must be 16-byte aligned";
      return DGREP_E_INVALID;
    }
    c->last_newline_ms = c->last_rebase_ms = 0.f;
    *c->h_bat_flag = UINT64_MAX;
    HIPCHK(hipMemcpyAsync(c->d_bat_begin, c->bat_begin.data(), (k + 1) * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemsetAsync(c->d_bat_lines, 0, k * 8, c->stream));
    HIPCHK(hipMemsetAsync(b.bad_split, 0xff, 8, c->stream));
    HIPCHK(hipEventRecord(c->evb0, c->stream));
    HIPCHK(batch_split_newlines(b, c->num_cus, c->stream));
    HIPCHK(hipEventRecord(c->evb1, c->stream));
    HIPCHK(hipMemcpyAsync(c->h_bat_flag, b.bad_split, 8, hipMemcpyDeviceToHost, c->stream));
  }
  int rc;
  if ((rc = scan_resident(c, d_packed, n, d_line, d_start, d_len, capacity, count)) != DGREP_OK) return rc;
  if (prepass) {
    // scan_resident waited for the stream unless it had nothing to scan
    if (n == 0 || (c->pat.flags & DGREP_DFA_MATCH_NONE)) HIPCHK(hipStreamSynchronize(c->stream));
    if (*c->h_bat_flag != UINT64_MAX) {
      c->err = "packed buffer: the byte after split " + std::to_string(*c->h_bat_flag) + " is not '\\n'";
      *count = 0;
      return DGREP_E_INVALID;
    }
    HIPCHK(hipEventElapsedTime(&c->last_newline_ms, c->evb0, c->evb1));
  }
  const uint64_t nrec = std::min(*count, capacity);
  HIPCHK(hipEventRecord(c->evb2, c->stream));
  // the ranges are searched in the scan's packed-buffer starts: before the rebase
  if (d_split_begin && *count <= capacity)
    HIPCHK(batch_split_ranges(b, d_start, nrec, d_split_begin, c->num_cus, c->stream));
  HIPCHK(batch_rebase(b, d_line, d_start, d_split, nrec, c->num_cus, c->stream));
  HIPCHK(hipEventRecord(c->evb3, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  HIPCHK(hipEventElapsedTime(&c->last_rebase_ms, c->evb2, c->evb3));
  return DGREP_OK;
}

extern "C" int dgrep_scan_batch_device(dgrep_ctx* c, const void* d_packed, size_t n_packed, const uint64_t* split_len,
                                       size_t nsplits, uint64_t* d_line_no, uint64_t* d_start, uint64_t* d_len,
                                       uint32_t* d_split, uint64_t* d_split_begin, uint64_t capacity,
                                       uint64_t* count) {
  if (count) *count = 0;
  if (!c || !count || !split_len || nsplits == 0 || nsplits > UINT32_MAX || (n_packed && !d_packed) ||
      (capacity && (!d_line_no || !d_start || !d_len || !d_split)))
    return DGREP_E_INVALID;
  uint64_t total = nsplits - 1;
  for (size_t i = 0; i < nsplits; ++i) {
    if (split_len[i] > UINT64_MAX - 1 - total) {
      c->err = "dgrep_scan_batch_device: the split lengths overflow";
      return DGREP_E_INVALID;
    }
    total += split_len[i];
  }
  if (total != n_packed) {
    c->err = "dgrep_scan_batch_device: n_packed must be the split lengths plus nsplits - 1 separators";
    return DGREP_E_INVALID;
  }
  if (!c->loaded) { c->err = "no DFA loaded"; return DGREP_E_NO_DFA; }
  HIPCHK(hipSetDevice(c->device));
  int rc;
  if ((rc = batch_setup(c, split_len, nsplits)) != DGREP_OK) return rc;
  rc = batch_resident(c, static_cast<const uint8_t*>(d_packed), n_packed, nsplits, d_line_no, d_start, d_len, d_split,
                      d_split_begin, capacity, count, true);
  if (rc == DGREP_OK) {
    c->ms_sum += c->last_ms;
    ++c->ms_scans;
  }
  return rc;
}

// Host splits -> packed ingest -> batch scan into the context's result arrays
// (d_res_line / start / len / split, and d_res_sbegin when `ranges`), grown and
// re-scanned once if the first guess at the record count was too small.
static int batch_scan_host(dgrep_ctx* c, const uint8_t* const* data, const size_t* n, size_t nsplits, size_t total,
                           bool ranges, uint64_t* count_out) {
  int rc;
  static_assert(sizeof(size_t) == sizeof(uint64_t), "split lengths are passed on as u64");
  if ((rc = batch_setup(c, reinterpret_cast<const uint64_t*>(n), nsplits)) != DGREP_OK) return rc;
  if (total) {
    if ((rc = grow(c, c->d_data, (uint64_t(total) + 63) & ~uint64_t(63))) != DGREP_OK) return rc;
    if ((rc = ingest_resident(c, data, n, nsplits, total)) != DGREP_OK) return rc;
  }
  if (ranges && (rc = grow(c, c->d_res_sbegin, uint64_t(nsplits) + 1)) != DGREP_OK) return rc;
  uint64_t want = std::max<uint64_t>(c->d_res_line.cap, std::max<uint64_t>(1024, total / 512));
  uint64_t count = 0;
  for (int attempt = 0; attempt < 2; ++attempt) {
    if ((rc = grow_results(c, want)) != DGREP_OK) return rc;
    if ((rc = grow(c, c->d_res_split, c->d_res_line.cap)) != DGREP_OK) return rc;
    if ((rc = batch_resident(c, c->d_data, total, nsplits, c->d_res_line, c->d_res_start, c->d_res_len, c->d_res_split,
                             ranges ? c->d_res_sbegin : nullptr, c->d_res_line.cap, &count, attempt == 0)) != DGREP_OK)
      return rc;
    if (count <= c->d_res_line.cap) break;
    want = count;
  }
  *count_out = count;
  return DGREP_OK;
}

extern "C" int dgrep_scan_batch(dgrep_ctx* c, const uint8_t* const* data, const size_t* n, size_t nsplits,
                                dgrep_batch_result* out) {
  if (out) memset(out, 0, sizeof *out);
  if (!c || !out || !data || !n || nsplits == 0 || nsplits > UINT32_MAX) return DGREP_E_INVALID;
  for (size_t i = 0; i < nsplits; ++i)
    if (n[i] && !data[i]) return DGREP_E_INVALID;
  size_t total = 0;
  if (!pack_total(n, nsplits, &total) || total == ~size_t(0)) {
    c->err = "dgrep_scan_batch: the split lengths overflow";
    return DGREP_E_INVALID;
  }
  if (!c->loaded) { c->err = "no DFA loaded"; return DGREP_E_NO_DFA; }
  HIPCHK(hipSetDevice(c->device));
  int rc;
  uint64_t count = 0;
  if ((rc = batch_scan_host(c, data, n, nsplits, total, true, &count)) != DGREP_OK) return rc;
  out->count = count;
  out->nsplits = nsplits;
  const size_t b = count * 8;
  rc = fetch_results(c, {{&out->split_begin, c->d_res_sbegin, (nsplits + 1) * 8, 0},
                         {&out->line_no, c->d_res_line, b, 0},
                         {&out->start, c->d_res_start, b, 0},
                         {&out->len, c->d_res_len, b, 0},
                         {&out->split, c->d_res_split, count * 4, 0}});
  if (rc == DGREP_E_NOMEM) dgrep_batch_result_free(out);
  return rc;
}

extern "C" void dgrep_batch_result_free(dgrep_batch_result* r) {
  if (!r) return;
  free(r->line_no);
  free(r->start);
  free(r->len);
  free(r->split);
  free(r->split_begin);
  memset(r, 0, sizeof *r);
}

extern "C" int dgrep_last_batch_ms(dgrep_ctx* c, float* newline_ms, float* rebase_ms) {
  if (!c || !newline_ms || !rebase_ms) return DGREP_E_INVALID;
  *newline_ms = c->last_newline_ms;
  *rebase_ms = c->last_rebase_ms;
  return DGREP_OK;
}

// ---- a split consumed in windows (kernels/window.h) --------------------------
// One map task per input file (map_reduce/worker.go:72-76) makes a split "one
// unbounded string per file". The windowed forms keep only two window buffers
// on the device: while the scan runs on one, the next piece is DMA'd into the
// other, behind the carried tail. Each window's completed lines are scanned by
// scan_resident as they are and their records rebased by the stream's running
// (byte_base, line_base), so the concatenated records are those of dgrep_scan
// on the concatenated bytes, for every cut.
struct dgrep_job;
// a job's flush or window: `total` encoded bytes at d_src, their cell ends at d_end, into the job's arena
static int job_append_rows(dgrep_job* j, const uint8_t* d_src, uint64_t total, const uint64_t* d_end, uint64_t nend,
                           bool running_max, uint64_t rows, uint64_t lines);

struct dgrep_stream {
  dgrep_ctx* c = nullptr;
  size_t window = 0;
  uint32_t flags = 0;
  uint64_t gen = 0;        // the context's load generation at open
  int status = DGREP_OK;   // a HIP error or out-of-memory mid-stream: every later call returns it
  bool finished = false;
  // the two window buffers; buf[cur][0 : fill) is the carried tail
  DevBuf<uint8_t> buf[2];
  int cur = 0;
  uint64_t fill = 0;
  uint64_t byte_base = 0, line_base = 0;
  // device: the cut pass's partials [3 kCutBlocks], its result [3], the gather's total [1]; pinned: the last four
  DevBuf<unsigned long long> d_cut;
  PinnedBuf<unsigned long long> h_cut;
  Event ev_c0, ev_c1;  // the cut pass
  Event ev_free[2];    // buffer b's last reader on the context stream
  Event ev_in;         // the last copy into buf[cur] on the copy stream
  // the call's records so far (device), and its values (host)
  DevBuf<uint64_t> d_line, d_start, d_len;
  DevBuf<uint64_t> d_voff;  // [acc_cap + 1], DGREP_STREAM_VALUES
  uint64_t acc_cap = 0, nrec = 0;
  DevBuf<uint8_t> d_values;  // one window's gathered lines
  DevBuf<uint8_t> d_gscratch;
  uint8_t* h_values = nullptr;
  uint64_t h_values_cap = 0, vbytes = 0;
  // dgrep_stream_stats
  uint64_t windows = 0, max_carry = 0;
  float cut_ms = 0.f;
  // the call's scan stats, summed over its windows
  dgrep_scan_stats agg{};
  float agg_ms = 0.f;
  // DGREP_STREAM_BOUNDED (kernels/carry.h): a line that outgrew the window is
  // folded into its DFA state. While `carrying`, the unfinished line is the
  // folded bytes [line_start, byte_base) of the stream, kept only as the state
  // in d_carry, plus the tail buf[cur][0 : fill).
  bool carrying = false;
  uint64_t line_start = 0;
  // device, one allocation: the walks' counters [2] u64, then the carried state
  // and the last walk's two verdicts, u32; pinned: the verdicts
  DevBuf<unsigned long long> d_carry;
  PinnedBuf<uint32_t> h_verdict;
  DevBuf<uint32_t> d_pairs;   // the walk's (guess, exit) scratch
  Event ev_w0, ev_w1;         // the last walk (bounded streams only)
  Event ev_v;                 // the verdicts' copy to the host
  bool walk_untimed = false;  // ev_w0 / ev_w1 are recorded and not yet added to walk_ms
  uint64_t folds = 0, folded_bytes = 0, chunks = 0;
  float walk_ms = 0.f;
  // A partition stream (dgrep_stream_open_partitions, kernels/encode_window.h):
  // every window's records are encoded where they lie, in the window buffer,
  // into d_enc -- one window's bytes at a time -- and copied to the host
  // accumulator as one row of cells. No record array is kept.
  bool parts = false;
  uint32_t nreduce = 0;
  uint32_t key_hash0 = 0, fname_json_len = 0;
  DevBuf<uint8_t> d_fname;  // the filename, JSON-escaped
  DevBuf<uint8_t> d_enc, d_pscratch;
  DevBuf<uint64_t> d_pbounds;  // [2 nreduce + 2]
  std::vector<uint64_t> h_pbounds;
  Event ev_e0, ev_e1;  // partition streams only
  // the call's rows so far (host)
  uint8_t* h_cells = nullptr;
  uint64_t h_cells_cap = 0, cell_bytes = 0;
  std::vector<uint64_t> cell_off;  // rows * nreduce + 1 once a row exists
  float call_encode_ms = 0.f;
  // dgrep_stream_partition_stats
  uint64_t rows = 0, out_bytes = 0, long_values = 0;
  float encode_ms = 0.f;
  // the window route of a job (dgrep_job_*): the rows go to the job's device
  // arena and their boundaries to its segment table, nothing to the host
  dgrep_job* job = nullptr;
};

static uint32_t* carry_state(dgrep_stream* s) { return reinterpret_cast<uint32_t*>(s->d_carry.p + 2); }
static uint32_t* carry_verdict(dgrep_stream* s) { return carry_state(s) + 1; }

static uint32_t sat_add32(uint32_t a, uint32_t b) { return uint32_t(std::min<uint64_t>(uint64_t(a) + b, UINT32_MAX)); }

static void win_stats_begin(dgrep_stream* s) {
  s->agg = dgrep_scan_stats{};
  s->agg.stepper = uint32_t(s->c->pat.step_kind);
  s->agg_ms = 0.f;
  s->call_encode_ms = 0.f;
}

// one window's scan (the context's stats) added to the call's
static void win_stats_add(dgrep_stream* s, uint64_t n) {
  const dgrep_scan_stats& w = s->c->stats;
  dgrep_scan_stats& a = s->agg;
  if (n) {
    a.stepper = w.stepper;
    a.lane_chunk = w.lane_chunk;
    a.lane_slots = w.lane_slots;
  }
  a.scan_attempts = sat_add32(a.scan_attempts, w.scan_attempts);
  a.long_guess_misses = sat_add32(a.long_guess_misses, w.long_guess_misses);
  a.long_segments = sat_add32(a.long_segments, w.long_segments);
  a.tiles += w.tiles;
  a.overflow_lanes += w.overflow_lanes;
  a.matches += w.matches;
  a.candidates += w.candidates;
  a.pending += w.pending;
  a.scan_ms += w.scan_ms;
  a.overflow_ms += w.overflow_ms;
  a.verify_ms += w.verify_ms;
  s->agg_ms += s->c->last_ms;
}

static void win_stats_end(dgrep_stream* s) {
  s->c->stats = s->agg;
  s->c->last_ms = s->agg_ms;
  if (s->parts) s->c->last_encode_ms = s->call_encode_ms;
}

// buf[b] holds at least `need` bytes (and the padding the kernels' aligned
// reads may touch); its first `keep` bytes survive a reallocation.
static int win_reserve(dgrep_stream* s, int b, uint64_t need, uint64_t keep) {
  dgrep_ctx* c = s->c;
  const uint64_t want = ((need + 255) & ~uint64_t(255)) + 64;
  if (s->buf[b].holds(want)) return DGREP_OK;
  // copies into the old buffer (the carried tail) are in order on the copy stream: it is drained first
  bool nomem = false;
  const hipError_t e = s->buf[b].regrow(want, keep, c->stream, &nomem, c->ing.copy_stream);
  if (nomem) {
    c->err = "window buffer: out of device memory (" + std::to_string(want) + " bytes)";
    return DGREP_E_NOMEM;
  }
  HIPCHK(e);
  return DGREP_OK;
}

// The ingest with the window completion contract: host bytes -> dst, all of
// it queued on the copy stream (ring or direct path as ingest_resident
// chooses), no host wait beyond the ring's slot reuse. Returns with the last
// copy queued and s->ev_in recorded behind it.
static int win_ingest(dgrep_stream* s, uint8_t* dst, const uint8_t* src, size_t len) {
  dgrep_ctx* c = s->c;
  IngestRing* r = &c->ing;
  if (ingest_direct(*r, len)) {
    INGCHK(ingest_direct_copy(r, &src, &len, 1, false, dst, len, r->copy_stream));
  } else {
    INGCHK(ingest_ring(r));
    INGCHK(ingest_pieces(r, &src, &len, 1, false, dst, len));
  }
  HIPCHK(hipEventRecord(s->ev_in, r->copy_stream));
  return DGREP_OK;
}

// the call's record arrays hold `need` records; the nrec there survive
static int win_acc_reserve(dgrep_stream* s, uint64_t need) {
  dgrep_ctx* c = s->c;
  if (need <= s->acc_cap) return DGREP_OK;
  const uint64_t cap = std::max<uint64_t>(need, std::max<uint64_t>(1024, 2 * s->acc_cap));
  const bool values = (s->flags & DGREP_STREAM_VALUES) != 0;
  // all or nothing: the new arrays are made first, and on a failure they go and the old ones stand
  DevBuf<uint64_t> fresh[4];
  DevBuf<uint64_t>* old[4] = {&s->d_line, &s->d_start, &s->d_len, &s->d_voff};
  const int arrays = values ? 4 : 3;
  for (int i = 0; i < arrays; ++i) {
    const uint64_t extra = i == 3 ? 1 : 0;
    const char* what = "";
    if (fresh[i].discard(cap + extra, &what) != hipSuccess) {
      (void)hipGetLastError();
      c->err = "windowed scan: out of device memory for " + std::to_string(cap) + " records";
      return DGREP_E_NOMEM;
    }
    if (old[i]->p && s->nrec)
      HIPCHK(hipMemcpyAsync(fresh[i], *old[i], (s->nrec + extra) * 8, hipMemcpyDeviceToDevice, c->stream));
  }
  HIPCHK(hipStreamSynchronize(c->stream));
  for (int i = 0; i < arrays; ++i) old[i]->swap(fresh[i]);  // (the old arrays go with `fresh`)
  s->acc_cap = cap;
  return DGREP_OK;
}

// The loaded pattern's plain DFA on the device, from the host copy
// dgrep_load_dfa kept: once per pattern, at the first fold.
static int carry_ensure(dgrep_ctx* c) {
  if (c->carry_ready) return DGREP_OK;
  const uint32_t S = c->pat.h_nstates, K = c->pat.h_nclasses, nl = c->pat.h_cls[uint8_t('\n')];
  const size_t ne = size_t(S) * K;
  const bool u32 = S > 65535;
  const std::vector<uint8_t> absorbing = carry_absorbing(c->pat.h_trans.data(), S, K, nl);
  std::vector<uint8_t> aux(256 + size_t(S));
  memcpy(aux.data(), c->pat.h_cls, 256);
  memcpy(aux.data() + 256, absorbing.data(), S);
  std::vector<uint16_t> t16;
  const void* src = c->pat.h_trans.data();
  size_t bytes = ne * 4;
  if (!u32) {
    t16.resize(ne);
    for (size_t i = 0; i < ne; ++i) t16[i] = uint16_t(c->pat.h_trans[i]);
    src = t16.data();
    bytes = ne * 2;
  }
  if (!c->dev.carry_trans) HIPCHK(hipMalloc(&c->dev.carry_trans, std::max<size_t>(bytes, 16)));
  if (!c->dev.carry_aux) HIPCHK(hipMalloc(reinterpret_cast<void**>(&c->dev.carry_aux), aux.size()));
  HIPCHK(hipMemcpy(c->dev.carry_trans, src, bytes, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(c->dev.carry_aux, aux.data(), aux.size(), hipMemcpyHostToDevice));
  CarryTable& t = c->carry;
  t.trans = c->dev.carry_trans;
  t.cls = c->dev.carry_aux;
  t.absorbing = c->dev.carry_aux + 256;
  t.nstates = S;
  t.nclasses = K;
  t.start = c->pat.h_start;
  t.start_m = c->pat.h_start_m;
  t.nl_class = nl;
  t.u32 = u32;
  carry_seeds(absorbing, S, c->pat.h_start, t.seed);
  c->carry_ready = true;
  return DGREP_OK;
}

// the last walk's device time, once the host knows it is done
static int carry_ms_take(dgrep_stream* s) {
  dgrep_ctx* c = s->c;
  if (!s->walk_untimed) return DGREP_OK;
  float ms = 0.f;
  HIPCHK(hipEventElapsedTime(&ms, s->ev_w0, s->ev_w1));
  s->walk_ms += ms;
  s->walk_untimed = false;
  return DGREP_OK;
}

// Queue the walk of d[0 : m) (no '\n' in it) from the carried state, or from
// `start` if no line is carried; the carried state becomes the walk's exit.
// want_verdict: the verdicts go to h_verdict, valid once ev_v is done. No host
// wait, unless the walk before was never waited for.
static int win_walk(dgrep_stream* s, const uint8_t* d, uint64_t m, bool want_verdict, bool dual) {
  dgrep_ctx* c = s->c;
  int rc;
  if ((rc = carry_ensure(c)) != DGREP_OK) return rc;
  if (s->walk_untimed) {
    HIPCHK(hipEventSynchronize(s->ev_w1));
    if ((rc = carry_ms_take(s)) != DGREP_OK) return rc;
  }
  const bool rows_in_lds = uint64_t(c->pat.h_nstates) * c->pat.h_nclasses * (c->carry.u32 ? 4 : 2) <= kCarryRowsLds;
  const CarryPlan plan = carry_plan(m, carry_lanes(m, uint64_t(std::max(c->num_cus, 1)), rows_in_lds));
  if ((rc = grow(c, s->d_pairs, carry_pairs_bytes(plan) / 4)) != DGREP_OK) return rc;
  CarryWalk w;
  w.data = d;
  w.m = m;
  w.state = carry_state(s);
  w.from_start = !s->carrying;
  w.verdict = want_verdict ? carry_verdict(s) : nullptr;
  w.dual = dual;
  w.pairs = s->d_pairs;
  w.counters = s->d_carry;
  HIPCHK(hipEventRecord(s->ev_w0, c->stream));
  HIPCHK(carry_walk(c->carry, w, plan, c->stream));
  HIPCHK(hipEventRecord(s->ev_w1, c->stream));
  s->walk_untimed = true;
  s->chunks += plan.nchunks;
  if (want_verdict) {
    HIPCHK(hipMemcpyAsync(s->h_verdict, carry_verdict(s), 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipEventRecord(s->ev_v, c->stream));
  }
  return DGREP_OK;
}

// A partition stream's window: the scan's records (the context's result arrays,
// in the window's coordinates) encoded from the window buffer d[0 : n) into
// d_enc, and the bytes appended to the call's rows. The buffer is still the
// stream's: the caller records ev_free behind this.
static int win_encode(dgrep_stream* s, const uint8_t* d, uint64_t n, uint64_t count) {
  dgrep_ctx* c = s->c;
  if (count >= (uint64_t(1) << 32)) {
    c->err = "partition stream: 2^32 or more matching lines in one window";
    return DGREP_E_UNSUPPORTED;
  }
  int rc;
  const uint32_t R = s->nreduce;
  WindowEncodeArgs a;
  a.e.data = d;
  a.e.n = n;
  a.e.line_no = c->d_res_line;
  a.e.start = c->d_res_start;
  a.e.len = c->d_res_len;
  a.e.count = count;
  a.e.fname_json = s->d_fname;
  a.e.fname_json_len = s->fname_json_len;
  a.e.key_hash0 = s->key_hash0;
  a.e.nreduce = R;
  a.line_base = s->line_base;
  a.long_value = c->long_value ? c->long_value : kLongValueDefault;
  size_t need = 0;
  HIPCHK(encode_window_partitions(a, nullptr, &need, nullptr, 0, nullptr, c->stream));
  if ((rc = grow(c, s->d_pscratch, need)) != DGREP_OK) return rc;
  uint64_t total = 0;
  for (int attempt = 0; attempt < 2; ++attempt) {
    size_t have = s->d_pscratch.cap;
    HIPCHK(hipEventRecord(s->ev_e0, c->stream));
    HIPCHK(encode_window_partitions(a, s->d_pscratch, &have, s->d_enc, s->d_enc.cap, s->d_pbounds, c->stream));
    HIPCHK(hipEventRecord(s->ev_e1, c->stream));
    if (s->job)  // the totals only: the offsets stay on the device
      HIPCHK(hipMemcpyAsync(s->h_pbounds.data() + 2 * size_t(R), s->d_pbounds + 2 * size_t(R), 16,
                            hipMemcpyDeviceToHost, c->stream));
    else
      HIPCHK(hipMemcpyAsync(s->h_pbounds.data(), s->d_pbounds, s->h_pbounds.size() * 8, hipMemcpyDeviceToHost,
                            c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, s->ev_e0, s->ev_e1));
    s->call_encode_ms += ms;
    s->encode_ms += ms;
    total = s->h_pbounds[2 * size_t(R)];
    if (total <= s->d_enc.cap) break;
    if (attempt == 1) {
      c->err = "partition stream: the window's encoded size changed between two passes";
      return DGREP_E_HIP;
    }
    // the one buffer of encoded bytes the device holds: this window's, with a sixteenth to spare
    // (a job's append kernel reads whole 16-byte vectors)
    const uint64_t want = s->job ? (total + total / 16 + 15) & ~uint64_t(15) : total + total / 16;
    if ((rc = grow(c, s->d_enc, want)) != DGREP_OK) return rc;
  }
  if (s->job) {
    ++s->rows;
    s->out_bytes += total;
    s->long_values += s->h_pbounds[2 * size_t(R) + 1];
    // the partitions lie in order and back to back, an empty one's range is (0, 0): the running maximum
    // of their ends are the row's cell boundaries
    return job_append_rows(s->job, s->d_enc, total, s->d_pbounds + R, R, true, 1, count);
  }
  if (s->cell_bytes + total > s->h_cells_cap) {
    const uint64_t cap = std::max<uint64_t>(s->cell_bytes + total, 2 * s->h_cells_cap);
    uint8_t* p = static_cast<uint8_t*>(realloc(s->h_cells, cap));
    if (!p) return DGREP_E_NOMEM;
    s->h_cells = p;
    s->h_cells_cap = cap;
  }
  HIPCHK(hipMemcpyAsync(s->h_cells + s->cell_bytes, s->d_enc, total, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  // the window's bytes are partition-major and contiguous: a cell ends where the next one begins
  if (s->cell_off.empty()) s->cell_off.push_back(0);
  uint64_t at = s->cell_bytes;
  for (uint32_t p = 0; p < R; ++p) {
    at += s->h_pbounds[R + p] - s->h_pbounds[p];
    s->cell_off.push_back(at);
  }
  if (at != s->cell_bytes + total) {
    c->err = "partition stream: the partitions' ranges do not add up to the window's bytes";
    return DGREP_E_HIP;
  }
  s->cell_bytes = at;
  ++s->rows;
  s->out_bytes += total;
  s->long_values += s->h_pbounds[2 * size_t(R) + 1];
  return DGREP_OK;
}

// One window's completed lines d[0 : n) (16-byte aligned; n may be 0, the one
// empty line): scan, then the records rebased and appended to the call's, then
// their bytes gathered. `splice` (a bounded stream that carries a line): the
// region's line 1, d[0 : head), is the end of the carried line; its walk is
// queued with both verdicts wanted. The scan judged the head as a line of its
// own: that record is dropped, and the carried line's takes its place if the
// walk from the carried state says so.
static int win_scan(dgrep_stream* s, const uint8_t* d, uint64_t n, bool splice = false, uint64_t head = 0) {
  dgrep_ctx* c = s->c;
  int rc;
  uint64_t count = 0;
  uint64_t want = std::max<uint64_t>(c->d_res_line.cap, std::max<uint64_t>(1024, n / 512));
  for (int attempt = 0; attempt < 2; ++attempt) {
    if ((rc = grow_results(c, want)) != DGREP_OK) return rc;
    if ((rc = scan_resident(c, d, n, c->d_res_line, c->d_res_start, c->d_res_len, c->d_res_line.cap, &count)) != DGREP_OK)
      return rc;
    if (count <= c->d_res_line.cap) break;
    want = count;
  }
  win_stats_add(s, n);
  ++s->windows;
  if (splice) {
    // the verdicts were queued before the scan: behind the scan's own host wait this one returns at once
    HIPCHK(hipEventSynchronize(s->ev_v));
    if ((rc = carry_ms_take(s)) != DGREP_OK) return rc;
    const uint64_t ins = s->h_verdict[0] ? 1 : 0, drop = s->h_verdict[1] ? 1 : 0;
    if (drop > count) {
      c->err = "bounded stream: the scan and the walk disagree on the carried line's end";
      return DGREP_E_HIP;
    }
    s->agg.matches = s->agg.matches - drop + ins;
    const uint64_t kept = count - drop;
    if (kept + ins == 0) return DGREP_OK;
    if ((rc = win_acc_reserve(s, s->nrec + kept + ins)) != DGREP_OK) return rc;
    if (ins)
      HIPCHK(carry_put_record(s->d_line + s->nrec, s->d_start + s->nrec, s->d_len + s->nrec, s->line_base + 1,
                              s->line_start, s->byte_base + head - s->line_start, c->stream));
    s->nrec += ins;
    HIPCHK(window_rebase_append(c->d_res_line + drop, c->d_res_start + drop, c->d_res_len + drop, kept, s->line_base,
                                s->byte_base, s->d_line + s->nrec, s->d_start + s->nrec, s->d_len + s->nrec,
                                c->num_cus, c->stream));
    s->nrec += kept;
    return DGREP_OK;  // a bounded stream returns no values
  }
  if (count == 0) return DGREP_OK;
  if (s->parts) return win_encode(s, d, n, count);
  if ((rc = win_acc_reserve(s, s->nrec + count)) != DGREP_OK) return rc;
  HIPCHK(window_rebase_append(c->d_res_line, c->d_res_start, c->d_res_len, count, s->line_base, s->byte_base,
                              s->d_line + s->nrec, s->d_start + s->nrec, s->d_len + s->nrec, c->num_cus, c->stream));
  if (s->flags & DGREP_STREAM_VALUES) {
    if (count >= (uint64_t(1) << 31)) {
      c->err = "windowed scan: 2^31 or more matching lines in one window";
      return DGREP_E_UNSUPPORTED;
    }
    // the lines lie apart in the region: their bytes sum to at most n
    if ((rc = grow(c, s->d_values, std::max<uint64_t>(n, 1))) != DGREP_OK) return rc;
    GatherArgs g;
    g.data = d;
    g.start = c->d_res_start;
    g.len = c->d_res_len;
    g.nrec = count;
    g.value_base = s->vbytes;
    g.value_off = s->d_voff + s->nrec;
    g.values = s->d_values;
    g.total = s->d_cut + 3 * kCutBlocks + 3;
    size_t need = 0;
    HIPCHK(window_gather(g, nullptr, &need, c->num_cus, c->stream));
    if ((rc = grow(c, s->d_gscratch, need)) != DGREP_OK) return rc;
    size_t have = s->d_gscratch.cap;
    HIPCHK(window_gather(g, s->d_gscratch, &have, c->num_cus, c->stream));
    HIPCHK(hipMemcpyAsync(s->h_cut + 3, g.total, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    const uint64_t wt = s->h_cut[3];
    if (wt > n) {
      c->err = "windowed scan: gathered more bytes than the window holds";
      return DGREP_E_HIP;
    }
    if (s->vbytes + wt > s->h_values_cap) {
      const uint64_t cap = std::max<uint64_t>(s->vbytes + wt, 2 * s->h_values_cap);
      uint8_t* p = static_cast<uint8_t*>(realloc(s->h_values, cap));
      if (!p) return DGREP_E_NOMEM;
      s->h_values = p;
      s->h_values_cap = cap;
    }
    if (wt) {
      HIPCHK(hipMemcpyAsync(s->h_values + s->vbytes, s->d_values, wt, hipMemcpyDeviceToHost, c->stream));
      HIPCHK(hipStreamSynchronize(c->stream));
    }
    s->vbytes += wt;
  }
  s->nrec += count;
  return DGREP_OK;
}

// The feed's bytes, in pieces of at most one window. Every piece is a window
// that is not the last: the cut pass finds the last '\n' of the carried tail
// plus the piece, the tail behind it is carried to the other buffer and the
// next piece's DMA queued behind the tail -- both before the host waits for
// this window's scan. Returns with every copy out of `data` done.
static int win_feed(dgrep_stream* s, const uint8_t* data, size_t n) {
  dgrep_ctx* c = s->c;
  int rc;
  size_t off = 0;
  uint64_t pending = std::min<uint64_t>(s->window, n);  // bytes queued behind the tail in buf[cur]
  if (pending) {
    if ((rc = win_reserve(s, s->cur, s->fill + pending, s->fill)) != DGREP_OK) return rc;
    if ((rc = win_ingest(s, s->buf[s->cur] + s->fill, data, pending)) != DGREP_OK) return rc;
    off = pending;
  }
  unsigned long long* const d_res = s->d_cut + 3 * kCutBlocks;
  while (pending) {
    const uint64_t F = s->fill + pending;
    HIPCHK(hipStreamWaitEvent(c->stream, s->ev_in, 0));
    HIPCHK(hipEventRecord(s->ev_c0, c->stream));
    HIPCHK(window_cut(s->buf[s->cur], F, s->fill, s->d_cut, d_res, c->num_cus, c->stream));
    HIPCHK(hipEventRecord(s->ev_c1, c->stream));
    HIPCHK(hipMemcpyAsync(s->h_cut, d_res, 24, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, s->ev_c0, s->ev_c1));
    s->cut_ms += ms;
    const uint64_t last1 = s->h_cut[0], nl = s->h_cut[1];
    if (last1 > F) {
      c->err = "windowed scan: the cut lies past the window";
      return DGREP_E_HIP;
    }
    const uint64_t next = std::min<uint64_t>(s->window, n - off);
    if ((rc = carry_ms_take(s)) != DGREP_OK) return rc;  // a walk queued before this window's cut is done
    if (last1 == 0 && (s->flags & DGREP_STREAM_BOUNDED) && F >= s->window) {
      // Fold: a full window and no line completed. Its bytes go into the
      // carried state and are forgotten; the next piece lands at the front of
      // the other buffer while the walk reads this one. No host wait.
      if ((rc = win_walk(s, s->buf[s->cur], F, false, false)) != DGREP_OK) return rc;
      HIPCHK(hipEventRecord(s->ev_free[s->cur], c->stream));
      if (!s->carrying) s->line_start = s->byte_base;
      s->carrying = true;
      s->byte_base += F;
      ++s->folds;
      s->folded_bytes += F;
      s->max_carry = std::max(s->max_carry, s->byte_base - s->line_start);
      const int o = s->cur ^ 1;
      HIPCHK(hipStreamWaitEvent(c->ing.copy_stream, s->ev_free[o], 0));
      if (next) {
        if ((rc = win_reserve(s, o, next, 0)) != DGREP_OK) return rc;
        if ((rc = win_ingest(s, s->buf[o], data + off, next)) != DGREP_OK) return rc;
        off += next;
      } else {
        HIPCHK(hipEventRecord(s->ev_in, c->ing.copy_stream));
      }
      s->cur = o;
      s->fill = 0;
      pending = next;
      continue;
    }
    if (last1 == 0) {
      // no line completed: all of it is the tail, and the next piece lands behind it
      s->fill = F;
      s->max_carry = std::max(s->max_carry, s->carrying ? s->byte_base + F - s->line_start : F);
      pending = next;
      if (next) {
        if ((rc = win_reserve(s, s->cur, F + next, F)) != DGREP_OK) return rc;
        if ((rc = win_ingest(s, s->buf[s->cur] + F, data + off, next)) != DGREP_OK) return rc;
        off += next;
      }
      continue;
    }
    const uint64_t cut = last1 - 1, tail = F - last1;
    // the line the carried tail began ends at the first '\n' behind the tail: its whole length was held
    if (s->fill && s->h_cut[2]) s->max_carry = std::max<uint64_t>(s->max_carry, s->h_cut[2] - 1);
    const int o = s->cur ^ 1;
    if ((rc = win_reserve(s, o, tail + next, 0)) != DGREP_OK) return rc;
    HIPCHK(hipStreamWaitEvent(c->ing.copy_stream, s->ev_free[o], 0));
    if (tail)
      HIPCHK(hipMemcpyAsync(s->buf[o], s->buf[s->cur] + last1, tail, hipMemcpyDeviceToDevice, c->ing.copy_stream));
    if (next) {
      if ((rc = win_ingest(s, s->buf[o] + tail, data + off, next)) != DGREP_OK) return rc;
      off += next;
    } else {
      HIPCHK(hipEventRecord(s->ev_in, c->ing.copy_stream));
    }
    if (s->carrying) {
      // The carried line ends in this window, at the first '\n' (the tail holds
      // none, so the first one behind it is the first one): walk its last bytes
      // from the carried state, and from `start` as the scan will.
      const uint64_t first1 = s->h_cut[2];
      if (first1 == 0 || first1 > last1) {
        c->err = "bounded stream: the carried line's end lies outside the window";
        return DGREP_E_HIP;
      }
      const uint64_t head = first1 - 1;
      if ((rc = win_walk(s, s->buf[s->cur], head, true, true)) != DGREP_OK) return rc;
      s->max_carry = std::max(s->max_carry, s->byte_base + head - s->line_start);
      if ((rc = win_scan(s, s->buf[s->cur], cut, true, head)) != DGREP_OK) return rc;
      s->carrying = false;
    } else if ((rc = win_scan(s, s->buf[s->cur], cut)) != DGREP_OK) {
      return rc;
    }
    HIPCHK(hipEventRecord(s->ev_free[s->cur], c->stream));
    s->byte_base += last1;
    s->line_base += nl;
    s->cur = o;
    s->fill = tail;
    s->max_carry = std::max(s->max_carry, tail);
    pending = next;
  }
  return DGREP_OK;
}

// the end of the stream: what is left is its last line (maybe the empty one)
static int win_finish(dgrep_stream* s) {
  dgrep_ctx* c = s->c;
  HIPCHK(hipStreamWaitEvent(c->stream, s->ev_in, 0));
  int rc;
  if (s->carrying) {
    // the last line is the carried one: its folded bytes, then the tail
    if ((rc = win_walk(s, s->buf[s->cur], s->fill, true, false)) != DGREP_OK) return rc;
    HIPCHK(hipEventSynchronize(s->ev_v));
    if ((rc = carry_ms_take(s)) != DGREP_OK) return rc;
    const uint64_t len = s->byte_base + s->fill - s->line_start;
    s->max_carry = std::max(s->max_carry, len);
    ++s->windows;
    if (s->h_verdict[0]) {
      if ((rc = win_acc_reserve(s, s->nrec + 1)) != DGREP_OK) return rc;
      HIPCHK(carry_put_record(s->d_line + s->nrec, s->d_start + s->nrec, s->d_len + s->nrec, s->line_base + 1,
                              s->line_start, len, c->stream));
      ++s->nrec;
      ++s->agg.matches;
    }
    s->carrying = false;
    s->finished = true;
    return DGREP_OK;
  }
  rc = win_scan(s, s->buf[s->cur], s->fill);
  if (rc == DGREP_OK) s->finished = true;
  return rc;
}

// The call's records (and values) to the host, malloc'd; the stream starts its
// next call's result empty.
static int win_collect(dgrep_stream* s, dgrep_stream_result* out) {
  dgrep_ctx* c = s->c;
  const uint64_t count = s->nrec;
  const bool values = (s->flags & DGREP_STREAM_VALUES) != 0;
  out->count = count;
  const size_t b = count * 8;
  const int rc = fetch_results(c, {{&out->line_no, s->d_line, b, 0},
                                   {&out->start, s->d_start, b, 0},
                                   {&out->len, s->d_len, b, 0},
                                   {&out->value_off, s->d_voff.p ? s->d_voff + 1 : nullptr, values ? b : 0, values ? 8u : 0u}});
  if (rc == DGREP_E_NOMEM) dgrep_stream_result_free(out);
  if (rc != DGREP_OK) return rc;
  if (values) {
    out->value_off[0] = 0;
    out->values = s->h_values;
    s->h_values = nullptr;
    s->h_values_cap = 0;
  }
  s->nrec = 0;
  s->vbytes = 0;
  return DGREP_OK;
}

static bool win_window_ok(size_t window_bytes) {
  return window_bytes >= 4096 && window_bytes <= (size_t(1) << 40) && window_bytes % 4096 == 0;
}

static int win_open(dgrep_ctx* c, size_t window_bytes, uint32_t flags, dgrep_stream** out) {
  dgrep_stream* s = new dgrep_stream();
  s->c = c;
  s->window = window_bytes;
  s->flags = flags;
  s->gen = c->load_gen;
  *out = s;  // kept on failure too: dgrep_stream_close frees what was made
  int rc;
  HIPCHK(c->ing.copy_stream.create());
  if ((rc = grow(c, s->d_cut, 3 * kCutBlocks + 4)) != DGREP_OK) return rc;
  HIPCHK(s->h_cut.alloc(4));
  HIPCHK(s->ev_c0.create());
  HIPCHK(s->ev_c1.create());
  for (Event* e : {&s->ev_free[0], &s->ev_free[1], &s->ev_in}) HIPCHK(e->create(hipEventDisableTiming));
  if (flags & DGREP_STREAM_BOUNDED) {
    if ((rc = grow(c, s->d_carry, 4)) != DGREP_OK) return rc;
    HIPCHK(hipMemsetAsync(s->d_carry, 0, 32, c->stream));
    HIPCHK(s->h_verdict.alloc(2));
    HIPCHK(s->ev_w0.create());
    HIPCHK(s->ev_w1.create());
    HIPCHK(s->ev_v.create(hipEventDisableTiming));
  }
  return DGREP_OK;
}

extern "C" void dgrep_stream_close(dgrep_stream* s) {
  if (!s) return;
  dgrep_ctx* c = s->c;
  (void)hipSetDevice(c->device);
  if (c->ing.copy_stream) (void)hipStreamSynchronize(c->ing.copy_stream);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  free(s->h_values);
  free(s->h_cells);
  delete s;
}

extern "C" void dgrep_stream_result_free(dgrep_stream_result* r) {
  if (!r) return;
  free(r->line_no);
  free(r->start);
  free(r->len);
  free(r->value_off);
  free(r->values);
  memset(r, 0, sizeof *r);
}

static const char kBoundedPartial[] =
    "a bounded stream carries an exact DFA state: a DGREP_DFA_PARTIAL pattern (over the compiler's state budget) "
    "has none past CAND";

extern "C" int dgrep_stream_open(dgrep_ctx* c, size_t window_bytes, uint32_t flags, dgrep_stream** out) {
  if (out) *out = nullptr;
  if (!c || !out || (flags & ~uint32_t(DGREP_STREAM_VALUES | DGREP_STREAM_BOUNDED))) return DGREP_E_INVALID;
  const bool bounded = (flags & DGREP_STREAM_BOUNDED) != 0;
  if (bounded && (flags & DGREP_STREAM_VALUES)) {
    c->err = "DGREP_STREAM_BOUNDED with DGREP_STREAM_VALUES: a folded line's bytes are gone";
    return DGREP_E_INVALID;
  }
  if (!win_window_ok(window_bytes)) {
    c->err = "window_bytes must be a multiple of 4096 in [4096, 2^40]";
    return DGREP_E_INVALID;
  }
  if (bounded && !c->loaded) {
    // whether a line's state can be carried is the pattern's property: without one the flag means nothing
    c->err = "DGREP_STREAM_BOUNDED needs a loaded pattern";
    return DGREP_E_INVALID;
  }
  if (!c->loaded) { c->err = "no DFA loaded"; return DGREP_E_NO_DFA; }
  if (bounded && (c->pat.flags & DGREP_DFA_PARTIAL)) {
    c->err = kBoundedPartial;
    return DGREP_E_UNSUPPORTED;
  }
  HIPCHK(hipSetDevice(c->device));
  const int rc = win_open(c, window_bytes, flags, out);
  if (rc != DGREP_OK) {
    dgrep_stream_close(*out);
    *out = nullptr;
  }
  return rc;
}

static const char kWantParts[] =
    "this is a partition stream (dgrep_stream_open_partitions): use dgrep_stream_feed_partitions / "
    "dgrep_stream_finish_partitions";
static const char kWantRecords[] =
    "this is a record stream (dgrep_stream_open): the _partitions calls need dgrep_stream_open_partitions";

// The checks every stream call makes before it touches the GPU.
static int win_enter(dgrep_stream* s, bool feeding) {
  dgrep_ctx* c = s->c;
  if (s->status != DGREP_OK) return s->status;
  if (s->finished) {
    c->err = feeding ? "dgrep_stream_feed after dgrep_stream_finish" : "dgrep_stream_finish called twice";
    return DGREP_E_INVALID;
  }
  if (s->gen != c->load_gen) {
    c->err = "a pattern was loaded while this stream was open: its records would mix two patterns";
    return DGREP_E_INVALID;
  }
  return DGREP_OK;
}

// a failure mid-stream leaves the stream unusable; nothing of the caller's is read after the return
static int win_fail(dgrep_stream* s, int rc) {
  if (rc == DGREP_OK) return rc;
  dgrep_ctx* c = s->c;
  const std::string msg = c->err;
  s->status = rc;
  if (c->ing.copy_stream) (void)hipStreamSynchronize(c->ing.copy_stream);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  (void)hipGetLastError();
  c->err = msg;
  return rc;
}

extern "C" int dgrep_stream_feed(dgrep_stream* s, const uint8_t* data, size_t n, dgrep_stream_result* out) {
  if (out) memset(out, 0, sizeof *out);
  if (!s || !out || (n && !data)) return DGREP_E_INVALID;
  dgrep_ctx* c = s->c;
  if (s->parts) { c->err = kWantParts; return DGREP_E_INVALID; }
  int rc;
  if ((rc = win_enter(s, true)) != DGREP_OK) return rc;
  win_stats_begin(s);
  if (n && !(c->pat.flags & DGREP_DFA_MATCH_NONE)) {
    HIPCHK(hipSetDevice(c->device));
    if ((rc = win_fail(s, win_feed(s, data, n))) != DGREP_OK) return rc;
    if ((rc = win_fail(s, win_collect(s, out))) != DGREP_OK) return rc;
  } else if (s->flags & DGREP_STREAM_VALUES) {
    if (!(out->value_off = static_cast<uint64_t*>(calloc(1, 8)))) return DGREP_E_NOMEM;
  }
  win_stats_end(s);
  return DGREP_OK;
}

extern "C" int dgrep_stream_finish(dgrep_stream* s, dgrep_stream_result* out) {
  if (out) memset(out, 0, sizeof *out);
  if (!s || !out) return DGREP_E_INVALID;
  dgrep_ctx* c = s->c;
  if (s->parts) { c->err = kWantParts; return DGREP_E_INVALID; }
  int rc;
  if ((rc = win_enter(s, false)) != DGREP_OK) return rc;
  win_stats_begin(s);
  if (!(c->pat.flags & DGREP_DFA_MATCH_NONE)) {
    HIPCHK(hipSetDevice(c->device));
    if ((rc = win_fail(s, win_finish(s))) != DGREP_OK) return rc;
    if ((rc = win_fail(s, win_collect(s, out))) != DGREP_OK) return rc;
  } else {
    s->finished = true;
    if ((s->flags & DGREP_STREAM_VALUES) && !(out->value_off = static_cast<uint64_t*>(calloc(1, 8))))
      return DGREP_E_NOMEM;
  }
  win_stats_end(s);
  return DGREP_OK;
}

extern "C" int dgrep_stream_stats(dgrep_stream* s, uint64_t* windows, uint64_t* data_bytes, uint64_t* max_carry,
                                  float* cut_ms) {
  if (!s) return DGREP_E_INVALID;
  if (windows) *windows = s->windows;
  if (data_bytes) *data_bytes = s->buf[0].cap + s->buf[1].cap;
  if (max_carry) *max_carry = s->max_carry;
  if (cut_ms) *cut_ms = s->cut_ms;
  return DGREP_OK;
}

extern "C" int dgrep_stream_carry_stats(dgrep_stream* s, uint64_t* folds, uint64_t* folded_bytes, uint64_t* chunks,
                                        uint64_t* guess_misses, float* walk_ms) {
  if (!s) return DGREP_E_INVALID;
  dgrep_ctx* c = s->c;
  unsigned long long ctr[2] = {0, 0};
  if (s->d_carry && (guess_misses || walk_ms)) {
    // the misses are counted on the device, and the last walk may still run
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipMemcpyAsync(ctr, s->d_carry, sizeof ctr, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    const int rc = carry_ms_take(s);
    if (rc != DGREP_OK) return rc;
  }
  if (folds) *folds = s->folds;
  if (folded_bytes) *folded_bytes = s->folded_bytes;
  if (chunks) *chunks = s->chunks;
  if (guess_misses) *guess_misses = ctr[1];
  if (walk_ms) *walk_ms = s->walk_ms;
  return DGREP_OK;
}

static int scan_windowed_flags(dgrep_ctx* c, const uint8_t* data, size_t n, size_t window_bytes, uint32_t flags,
                               dgrep_result* out);

extern "C" int dgrep_scan_windowed(dgrep_ctx* c, const uint8_t* data, size_t n, size_t window_bytes,
                                   dgrep_result* out) {
  return scan_windowed_flags(c, data, n, window_bytes, 0, out);
}

extern "C" int dgrep_scan_bounded(dgrep_ctx* c, const uint8_t* data, size_t n, size_t window_bytes,
                                  dgrep_result* out) {
  return scan_windowed_flags(c, data, n, window_bytes, DGREP_STREAM_BOUNDED, out);
}

static int scan_windowed_flags(dgrep_ctx* c, const uint8_t* data, size_t n, size_t window_bytes, uint32_t flags,
                               dgrep_result* out) {
  if (out) memset(out, 0, sizeof *out);
  if (!c || !out || (n && !data)) return DGREP_E_INVALID;
  if (!win_window_ok(window_bytes)) {
    c->err = "window_bytes must be a multiple of 4096 in [4096, 2^40]";
    return DGREP_E_INVALID;
  }
  if (!c->loaded) { c->err = "no DFA loaded"; return DGREP_E_NO_DFA; }
  if ((flags & DGREP_STREAM_BOUNDED) && (c->pat.flags & DGREP_DFA_PARTIAL)) {
    c->err = kBoundedPartial;
    return DGREP_E_UNSUPPORTED;
  }
  HIPCHK(hipSetDevice(c->device));
  dgrep_stream* s = nullptr;
  int rc = win_open(c, window_bytes, flags, &s);
  dgrep_stream_result r;
  memset(&r, 0, sizeof r);
  win_stats_begin(s);
  if (rc == DGREP_OK && !(c->pat.flags & DGREP_DFA_MATCH_NONE)) {
    if (n) rc = win_fail(s, win_feed(s, data, n));
    if (rc == DGREP_OK) rc = win_fail(s, win_finish(s));
    if (rc == DGREP_OK) rc = win_fail(s, win_collect(s, &r));
  }
  if (rc == DGREP_OK) win_stats_end(s);
  const std::string msg = c->err;
  dgrep_stream_close(s);  // the context holds no stream when the call returns
  c->err = msg;
  if (rc != DGREP_OK) return rc;
  out->count = r.count;
  out->line_no = r.line_no;
  out->start = r.start;
  out->len = r.len;
  return DGREP_OK;
}

// ---- the windowed map task: a stream that returns partition cells ------------
// The call's rows to the caller, malloc'd; the stream starts its next call's
// result empty.
static int win_collect_parts(dgrep_stream* s, dgrep_batch_partitions* out) {
  const uint64_t ncell = s->cell_off.empty() ? 0 : s->cell_off.size() - 1;
  out->nreduce = s->nreduce;
  out->nsplits = ncell / s->nreduce;
  out->cell_off = static_cast<uint64_t*>(calloc(ncell + 1, 8));
  if (!out->cell_off) return DGREP_E_NOMEM;
  if (ncell) memcpy(out->cell_off, s->cell_off.data(), (ncell + 1) * 8);
  out->total = s->cell_bytes;
  if (s->cell_bytes) {
    out->bytes = s->h_cells;
    s->h_cells = nullptr;
    s->h_cells_cap = 0;
  }
  s->cell_off.clear();
  s->cell_bytes = 0;
  return DGREP_OK;
}

// the argument checks of the partition forms that need no GPU; the message is set
static int parts_args_ok(dgrep_ctx* c, size_t window_bytes, const char* filename, size_t fn, uint32_t nreduce) {
  if (!win_window_ok(window_bytes)) {
    c->err = "window_bytes must be a multiple of 4096 in [4096, 2^40]";
    return DGREP_E_INVALID;
  }
  if (fn && !filename) { c->err = "filename is NULL with fn != 0"; return DGREP_E_INVALID; }
  if (nreduce == 0 || nreduce > 65535) { c->err = "nreduce must be 1..65535"; return DGREP_E_INVALID; }
  if (!c->loaded) { c->err = "no DFA loaded"; return DGREP_E_NO_DFA; }
  return DGREP_OK;
}

static int win_open_parts(dgrep_ctx* c, size_t window_bytes, const char* filename, size_t fn, uint32_t nreduce,
                          dgrep_stream** out) {
  int rc = win_open(c, window_bytes, 0, out);
  if (rc != DGREP_OK) return rc;
  dgrep_stream* s = *out;
  s->parts = true;
  s->nreduce = nreduce;
  const uint8_t* fname = reinterpret_cast<const uint8_t*>(filename);
  const uint64_t fj = json_escape_host(fname, fn, nullptr);
  if (fj >= (uint64_t(1) << 31)) { c->err = "filename too long"; return DGREP_E_INVALID; }
  std::vector<uint8_t> fjson(fj + 1);
  json_escape_host(fname, fn, fjson.data());
  s->fname_json_len = uint32_t(fj);
  s->key_hash0 = key_prefix_hash(fname, fn);
  if ((rc = grow(c, s->d_fname, fj + 1)) != DGREP_OK) return rc;
  HIPCHK(hipMemcpy(s->d_fname, fjson.data(), fj + 1, hipMemcpyHostToDevice));
  s->h_pbounds.assign(2 * size_t(nreduce) + 2, 0);
  if ((rc = grow(c, s->d_pbounds, s->h_pbounds.size())) != DGREP_OK) return rc;
  HIPCHK(s->ev_e0.create());
  HIPCHK(s->ev_e1.create());
  return DGREP_OK;
}

extern "C" int dgrep_stream_open_partitions(dgrep_ctx* c, size_t window_bytes, const char* filename, size_t fn,
                                            uint32_t nreduce, dgrep_stream** out) {
  if (out) *out = nullptr;
  if (!c || !out) return DGREP_E_INVALID;
  int rc;
  if ((rc = parts_args_ok(c, window_bytes, filename, fn, nreduce)) != DGREP_OK) return rc;
  HIPCHK(hipSetDevice(c->device));
  rc = win_open_parts(c, window_bytes, filename, fn, nreduce, out);
  if (rc != DGREP_OK) {
    const std::string msg = c->err;
    dgrep_stream_close(*out);
    c->err = msg;
    *out = nullptr;
  }
  return rc;
}

// an empty result: no row, the single offset 0
static int parts_empty(uint32_t nreduce, dgrep_batch_partitions* out) {
  out->nreduce = nreduce;
  return (out->cell_off = static_cast<uint64_t*>(calloc(1, 8))) ? DGREP_OK : DGREP_E_NOMEM;
}

extern "C" int dgrep_stream_feed_partitions(dgrep_stream* s, const uint8_t* data, size_t n,
                                            dgrep_batch_partitions* out) {
  if (out) memset(out, 0, sizeof *out);
  if (!s || !out || (n && !data)) return DGREP_E_INVALID;
  dgrep_ctx* c = s->c;
  if (!s->parts) { c->err = kWantRecords; return DGREP_E_INVALID; }
  int rc;
  if ((rc = win_enter(s, true)) != DGREP_OK) return rc;
  win_stats_begin(s);
  if (n && !(c->pat.flags & DGREP_DFA_MATCH_NONE)) {
    HIPCHK(hipSetDevice(c->device));
    if ((rc = win_fail(s, win_feed(s, data, n))) != DGREP_OK) return rc;
    if ((rc = win_fail(s, win_collect_parts(s, out))) != DGREP_OK) return rc;
  } else if ((rc = parts_empty(s->nreduce, out)) != DGREP_OK) {
    return rc;
  }
  win_stats_end(s);
  return DGREP_OK;
}

extern "C" int dgrep_stream_finish_partitions(dgrep_stream* s, dgrep_batch_partitions* out) {
  if (out) memset(out, 0, sizeof *out);
  if (!s || !out) return DGREP_E_INVALID;
  dgrep_ctx* c = s->c;
  if (!s->parts) { c->err = kWantRecords; return DGREP_E_INVALID; }
  int rc;
  if ((rc = win_enter(s, false)) != DGREP_OK) return rc;
  win_stats_begin(s);
  if (!(c->pat.flags & DGREP_DFA_MATCH_NONE)) {
    HIPCHK(hipSetDevice(c->device));
    if ((rc = win_fail(s, win_finish(s))) != DGREP_OK) return rc;
    if ((rc = win_fail(s, win_collect_parts(s, out))) != DGREP_OK) return rc;
  } else {
    s->finished = true;
    if ((rc = parts_empty(s->nreduce, out)) != DGREP_OK) return rc;
  }
  win_stats_end(s);
  return DGREP_OK;
}

extern "C" int dgrep_stream_partition_stats(dgrep_stream* s, uint64_t* rows, uint64_t* out_bytes,
                                            uint64_t* long_values, uint64_t* enc_device_bytes, float* encode_ms) {
  if (!s) return DGREP_E_INVALID;
  if (rows) *rows = s->rows;
  if (out_bytes) *out_bytes = s->out_bytes;
  if (long_values) *long_values = s->long_values;
  if (enc_device_bytes) *enc_device_bytes = s->d_enc.cap;
  if (encode_ms) *encode_ms = s->encode_ms;
  return DGREP_OK;
}

extern "C" int dgrep_map_partitions_windowed(dgrep_ctx* c, const uint8_t* data, size_t n, size_t window_bytes,
                                             const char* filename, size_t fn, uint32_t nreduce,
                                             dgrep_batch_partitions* out) {
  if (out) memset(out, 0, sizeof *out);
  if (!c || !out || (n && !data)) return DGREP_E_INVALID;
  int rc;
  if ((rc = parts_args_ok(c, window_bytes, filename, fn, nreduce)) != DGREP_OK) return rc;
  if (c->pat.flags & DGREP_DFA_MATCH_NONE) {
    c->stats = dgrep_scan_stats{};
    c->stats.stepper = uint32_t(c->pat.step_kind);
    c->last_ms = c->last_encode_ms = 0.f;
    return parts_empty(nreduce, out);
  }
  HIPCHK(hipSetDevice(c->device));
  dgrep_stream* s = nullptr;
  rc = win_open_parts(c, window_bytes, filename, fn, nreduce, &s);
  win_stats_begin(s);
  if (rc == DGREP_OK && n) rc = win_fail(s, win_feed(s, data, n));
  if (rc == DGREP_OK) rc = win_fail(s, win_finish(s));  // at most one more row, behind the feed's
  if (rc == DGREP_OK) rc = win_fail(s, win_collect_parts(s, out));
  if (rc == DGREP_OK) win_stats_end(s);
  const std::string msg = c->err;
  dgrep_stream_close(s);  // the context holds no stream when the call returns
  c->err = msg;
  if (rc != DGREP_OK) dgrep_batch_partitions_free(out);
  return rc;
}

// ---- partition + intermediate writer (map_reduce/worker.go:13-17,78-109) ----
static int encode_resident(dgrep_ctx* c, const uint8_t* d_data, uint64_t n, const uint64_t* d_line, const uint64_t* d_start,
                           const uint64_t* d_len, uint64_t count, const char* filename, size_t fn, uint32_t nreduce,
                           uint8_t* d_out, uint64_t out_cap, uint64_t* begin, uint64_t* end, uint64_t* total) {
  if (nreduce == 0 || nreduce > 65535) { c->err = "nreduce must be 1..65535"; return DGREP_E_INVALID; }
  if (count >= (uint64_t(1) << 32)) { c->err = "more than 2^32-1 records"; return DGREP_E_UNSUPPORTED; }
  int rc;
  const uint8_t* fname = reinterpret_cast<const uint8_t*>(filename);
  const uint64_t fj = json_escape_host(fname, fn, nullptr);
  if (fj >= (uint64_t(1) << 31)) { c->err = "filename too long"; return DGREP_E_INVALID; }
  std::vector<uint8_t> fjson(fj + 1);
  json_escape_host(fname, fn, fjson.data());
  if ((rc = grow(c, c->d_fname, fj + 1)) != DGREP_OK) return rc;
  HIPCHK(hipMemcpyAsync(c->d_fname, fjson.data(), fj + 1, hipMemcpyHostToDevice, c->stream));
  if ((rc = grow(c, c->d_bounds, 2 * uint64_t(nreduce) + 3)) != DGREP_OK) return rc;
  EncodeArgs a;
  a.data = d_data;
  a.n = n;
  a.line_no = d_line;
  a.start = d_start;
  a.len = d_len;
  a.count = count;
  a.fname_json = c->d_fname;
  a.fname_json_len = uint32_t(fj);
  a.key_hash0 = key_prefix_hash(fname, fn);
  a.nreduce = nreduce;
  const uint32_t long_value = c->long_value ? c->long_value : kLongValueResidentDefault;
  size_t need = 0;
  HIPCHK(encode_partitions(a, long_value, nullptr, &need, nullptr, 0, nullptr, c->stream));
  if ((rc = grow(c, c->d_enc_scratch, need)) != DGREP_OK) return rc;
  size_t have = c->d_enc_scratch.cap;
  HIPCHK(hipEventRecord(c->ev0, c->stream));
  HIPCHK(encode_partitions(a, long_value, c->d_enc_scratch, &have, d_out, out_cap, c->d_bounds, c->stream));
  HIPCHK(hipEventRecord(c->ev1, c->stream));
  std::vector<uint64_t> b(2 * size_t(nreduce) + 3);  // the long values and their chunks ride back with the bounds
  HIPCHK(hipMemcpyAsync(b.data(), c->d_bounds, b.size() * 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  HIPCHK(hipEventElapsedTime(&c->last_encode_ms, c->ev0, c->ev1));
  for (uint32_t p = 0; p < nreduce; ++p) {
    begin[p] = b[p];
    end[p] = b[nreduce + p];
  }
  *total = b[2 * size_t(nreduce)];
  c->enc_stats.records = count;
  c->enc_stats.long_values = b[2 * size_t(nreduce) + 1];
  c->enc_stats.long_chunks = b[2 * size_t(nreduce) + 2];
  return DGREP_OK;
}

extern "C" int dgrep_encode_device(dgrep_ctx* c, const void* d_data, size_t n, const uint64_t* d_line_no,
                                   const uint64_t* d_start, const uint64_t* d_len, uint64_t count,
                                   const char* filename, size_t fn, uint32_t nreduce, void* d_out, uint64_t out_cap,
                                   uint64_t* part_begin, uint64_t* part_end, uint64_t* total) {
  if (!c || !part_begin || !part_end || !total || (fn && !filename) || (count && (!d_line_no || !d_start || !d_len)) ||
      (n && !d_data) || (out_cap && !d_out))
    return DGREP_E_INVALID;
  HIPCHK(hipSetDevice(c->device));
  return encode_resident(c, static_cast<const uint8_t*>(d_data), n, d_line_no, d_start, d_len, count, filename, fn,
                         nreduce, static_cast<uint8_t*>(d_out), out_cap, part_begin, part_end, total);
}

extern "C" int dgrep_map_partitions(dgrep_ctx* c, const uint8_t* data, size_t n, const char* filename, size_t fn,
                                    uint32_t nreduce, dgrep_partitions* out) {
  if (!c || !out || (n && !data) || (fn && !filename) || nreduce == 0) return DGREP_E_INVALID;
  memset(out, 0, sizeof *out);
  if (!c->loaded) { c->err = "no DFA loaded"; return DGREP_E_NO_DFA; }
  HIPCHK(hipSetDevice(c->device));
  uint64_t count = 0;
  int rc;
  if ((rc = scan_host(c, data, n, &count)) != DGREP_OK) return rc;
  out->nreduce = nreduce;
  out->begin = static_cast<uint64_t*>(calloc(nreduce, 8));
  out->end = static_cast<uint64_t*>(calloc(nreduce, 8));
  if (!out->begin || !out->end) { dgrep_partitions_free(out); return DGREP_E_NOMEM; }
  const uint8_t* dd = c->d_data ? c->d_data : reinterpret_cast<const uint8_t*>(c->d_counters.p);
  uint64_t total = 0;
  for (int attempt = 0; attempt < 2; ++attempt) {
    if ((rc = encode_resident(c, dd, c->d_data ? n : 0, c->d_res_line, c->d_res_start, c->d_res_len, count, filename,
                              fn, nreduce,
                              c->d_enc_out, c->d_enc_out.cap, out->begin, out->end, &total)) != DGREP_OK) {
      dgrep_partitions_free(out);
      return rc;
    }
    if (total <= c->d_enc_out.cap) break;
    if ((rc = grow(c, c->d_enc_out, total + total / 16)) != DGREP_OK) {
      dgrep_partitions_free(out);
      return rc;
    }
  }
  out->total = total;
  if (total) {
    out->bytes = static_cast<uint8_t*>(malloc(total));
    if (!out->bytes) { dgrep_partitions_free(out); return DGREP_E_NOMEM; }
    HIPCHK(hipMemcpyAsync(out->bytes, c->d_enc_out, total, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
  }
  return DGREP_OK;
}

extern "C" void dgrep_partitions_free(dgrep_partitions* p) {
  if (!p) return;
  free(p->begin);
  free(p->end);
  free(p->bytes);
  memset(p, 0, sizeof *p);
}

// ---- partition + intermediate writer over a batch (kernels/encode_batch.h) ----
// The host image of the device filename table: name_off [k + 1] u64, then the
// FNV-1a prefix states [k] u32, then every name JSON-escaped, concatenated.
static int build_name_table(dgrep_ctx* c, const char* const* filename, const size_t* fn, size_t k,
                            std::vector<uint8_t>* img) {
  const size_t off_bytes = (k + 1) * 8, hash_bytes = k * 4;
  std::vector<uint64_t> off(k + 1);
  std::vector<uint32_t> hash(k);
  std::vector<uint8_t> esc;
  img->assign(off_bytes + hash_bytes, 0);
  for (size_t i = 0; i < k; ++i) {
    const uint8_t* f = reinterpret_cast<const uint8_t*>(filename[i]);
    if (fn[i] >= (size_t(1) << 31)) { c->err = "filename too long"; return DGREP_E_INVALID; }
    off[i] = img->size() - off_bytes - hash_bytes;
    hash[i] = key_prefix_hash(f, fn[i]);
    size_t plain = 0;  // the usual name has nothing to escape: copied as it is
    while (plain < fn[i] && f[plain] >= 0x20 && f[plain] < 0x80 && f[plain] != '"' && f[plain] != '\\' &&
           f[plain] != '<' && f[plain] != '>' && f[plain] != '&')
      ++plain;
    if (plain == fn[i]) {
      img->insert(img->end(), f, f + fn[i]);
      continue;
    }
    const uint64_t fj = json_escape_host(f, fn[i], nullptr);
    if (fj >= (uint64_t(1) << 31)) { c->err = "filename too long"; return DGREP_E_INVALID; }
    esc.resize(fj);
    json_escape_host(f, fn[i], esc.data());
    img->insert(img->end(), esc.begin(), esc.end());
  }
  off[k] = img->size() - off_bytes - hash_bytes;
  memcpy(img->data(), off.data(), off_bytes);
  memcpy(img->data() + off_bytes, hash.data(), hash_bytes);
  return DGREP_OK;
}

// Records of a batch scan over P (n bytes at d_packed, k splits, begin[] in
// c->bat_begin) -> every cell's lines in d_out; cell_off (host, k * nreduce + 1;
// nullptr: the offsets stay on the device in c->d_bat_cells, only the total is read).
static int encode_batch_resident(dgrep_ctx* c, const uint8_t* d_packed, uint64_t n, uint64_t k, const uint64_t* d_line,
                                 const uint64_t* d_start, const uint64_t* d_len, const uint32_t* d_split,
                                 uint64_t count, const std::vector<uint8_t>& names, uint32_t nreduce, uint8_t* d_out,
                                 uint64_t out_cap, uint64_t* cell_off, uint64_t* total) {
  const uint64_t cells = k * uint64_t(nreduce);
  *total = 0;
  c->enc_stats = dgrep_encode_stats{};
  if (count == 0) {
    if (cell_off) memset(cell_off, 0, (cells + 1) * 8);
    c->last_encode_ms = 0.f;
    return DGREP_OK;
  }
  int rc;
  if ((rc = grow(c, c->d_bat_names, names.size())) != DGREP_OK) return rc;
  if ((rc = grow(c, c->d_bat_cells, cells + 3)) != DGREP_OK) return rc;
  HIPCHK(hipMemcpyAsync(c->d_bat_begin, c->bat_begin.data(), (k + 1) * 8, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(c->d_bat_names, names.data(), names.size(), hipMemcpyHostToDevice, c->stream));
  EncodeBatchArgs a;
  a.data = d_packed;
  a.n = n;
  a.begin = c->d_bat_begin;
  a.k = k;
  a.line_no = d_line;
  a.start = d_start;
  a.len = d_len;
  a.split = d_split;
  a.count = count;
  a.name_off = reinterpret_cast<const uint64_t*>(c->d_bat_names.p);
  a.name_hash = reinterpret_cast<const uint32_t*>(c->d_bat_names + (k + 1) * 8);
  a.names = c->d_bat_names + (k + 1) * 8 + k * 4;
  a.nreduce = nreduce;
  const uint32_t long_value = c->long_value ? c->long_value : kLongValueResidentDefault;
  size_t need = 0;
  HIPCHK(encode_batch(a, long_value, nullptr, &need, nullptr, 0, nullptr, c->stream));
  if ((rc = grow(c, c->d_enc_scratch, need)) != DGREP_OK) return rc;
  size_t have = c->d_enc_scratch.cap;
  HIPCHK(hipEventRecord(c->ev0, c->stream));
  HIPCHK(encode_batch(a, long_value, c->d_enc_scratch, &have, d_out, out_cap, c->d_bat_cells, c->stream));
  HIPCHK(hipEventRecord(c->ev1, c->stream));
  uint64_t long_stats[2] = {0, 0};  // the long values and their chunks ride back with the offsets
  HIPCHK(hipMemcpyAsync(long_stats, c->d_bat_cells + cells + 1, 16, hipMemcpyDeviceToHost, c->stream));
  if (cell_off) HIPCHK(hipMemcpyAsync(cell_off, c->d_bat_cells, (cells + 1) * 8, hipMemcpyDeviceToHost, c->stream));
  else HIPCHK(hipMemcpyAsync(total, c->d_bat_cells + cells, 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  HIPCHK(hipEventElapsedTime(&c->last_encode_ms, c->ev0, c->ev1));
  if (cell_off) *total = cell_off[cells];
  c->enc_stats.records = count;
  c->enc_stats.long_values = long_stats[0];
  c->enc_stats.long_chunks = long_stats[1];
  return DGREP_OK;
}

// the argument checks the two batch-encode forms share (after their own)
static int encode_batch_args(dgrep_ctx* c, const char* const* filename, const size_t* fn, size_t nsplits,
                             uint32_t nreduce) {
  if (!filename || !fn) return DGREP_E_INVALID;
  if (nreduce == 0 || nreduce > 65535) { c->err = "nreduce must be 1..65535"; return DGREP_E_INVALID; }
  for (size_t i = 0; i < nsplits; ++i)
    if (fn[i] && !filename[i]) return DGREP_E_INVALID;
  return DGREP_OK;
}

extern "C" int dgrep_encode_batch_device(dgrep_ctx* c, const void* d_packed, size_t n_packed,
                                         const uint64_t* split_len, size_t nsplits, const uint64_t* d_line_no,
                                         const uint64_t* d_start, const uint64_t* d_len, const uint32_t* d_split,
                                         uint64_t count, const char* const* filename, const size_t* fn,
                                         uint32_t nreduce, void* d_out, uint64_t out_cap, uint64_t* cell_off,
                                         uint64_t* total) {
  if (total) *total = 0;
  if (!c || !total || !cell_off || !split_len || nsplits == 0 || nsplits > UINT32_MAX || (n_packed && !d_packed) ||
      (count && (!d_line_no || !d_start || !d_len || !d_split)) || (out_cap && !d_out))
    return DGREP_E_INVALID;
  int rc;
  if ((rc = encode_batch_args(c, filename, fn, nsplits, nreduce)) != DGREP_OK) return rc;
  uint64_t sum = nsplits - 1;
  for (size_t i = 0; i < nsplits; ++i) {
    if (split_len[i] > UINT64_MAX - 1 - sum) {
      c->err = "dgrep_encode_batch_device: the split lengths overflow";
      return DGREP_E_INVALID;
    }
    sum += split_len[i];
  }
  if (sum != n_packed) {
    c->err = "dgrep_encode_batch_device: n_packed must be the split lengths plus nsplits - 1 separators";
    return DGREP_E_INVALID;
  }
  if (uint64_t(nsplits) * nreduce >= (uint64_t(1) << 32)) {
    c->err = "dgrep_encode_batch_device: nsplits * nreduce must be below 2^32 cells";
    return DGREP_E_UNSUPPORTED;
  }
  if (count >= (uint64_t(1) << 32)) { c->err = "more than 2^32-1 records"; return DGREP_E_UNSUPPORTED; }
  std::vector<uint8_t> names;
  if ((rc = build_name_table(c, filename, fn, nsplits, &names)) != DGREP_OK) return rc;
  HIPCHK(hipSetDevice(c->device));
  if ((rc = batch_setup(c, split_len, nsplits)) != DGREP_OK) return rc;
  return encode_batch_resident(c, static_cast<const uint8_t*>(d_packed), n_packed, nsplits, d_line_no, d_start, d_len,
                               d_split, count, names, nreduce, static_cast<uint8_t*>(d_out), out_cap, cell_off, total);
}

extern "C" int dgrep_map_partitions_batch(dgrep_ctx* c, const uint8_t* const* data, const size_t* n,
                                          const char* const* filename, const size_t* fn, size_t nsplits,
                                          uint32_t nreduce, dgrep_batch_partitions* out) {
  if (out) memset(out, 0, sizeof *out);
  if (!c || !out || !data || !n || nsplits == 0 || nsplits > UINT32_MAX) return DGREP_E_INVALID;
  int rc;
  if ((rc = encode_batch_args(c, filename, fn, nsplits, nreduce)) != DGREP_OK) return rc;
  for (size_t i = 0; i < nsplits; ++i)
    if (n[i] && !data[i]) return DGREP_E_INVALID;
  size_t total_in = 0;
  if (!pack_total(n, nsplits, &total_in) || total_in == ~size_t(0)) {
    c->err = "dgrep_map_partitions_batch: the split lengths overflow";
    return DGREP_E_INVALID;
  }
  if (uint64_t(nsplits) * nreduce >= (uint64_t(1) << 32)) {
    c->err = "dgrep_map_partitions_batch: nsplits * nreduce must be below 2^32 cells";
    return DGREP_E_UNSUPPORTED;
  }
  if (!c->loaded) { c->err = "no DFA loaded"; return DGREP_E_NO_DFA; }
  std::vector<uint8_t> names;
  if ((rc = build_name_table(c, filename, fn, nsplits, &names)) != DGREP_OK) return rc;
  HIPCHK(hipSetDevice(c->device));
  uint64_t count = 0;
  if ((rc = batch_scan_host(c, data, n, nsplits, total_in, false, &count)) != DGREP_OK) return rc;
  if (count >= (uint64_t(1) << 32)) { c->err = "more than 2^32-1 records"; return DGREP_E_UNSUPPORTED; }
  const uint64_t cells = uint64_t(nsplits) * nreduce;
  out->cell_off = static_cast<uint64_t*>(calloc(cells + 1, 8));
  if (!out->cell_off) return DGREP_E_NOMEM;
  uint64_t total = 0;
  for (int attempt = 0; attempt < 2; ++attempt) {
    if ((rc = encode_batch_resident(c, c->d_data, total_in, nsplits, c->d_res_line, c->d_res_start, c->d_res_len,
                                    c->d_res_split, count, names, nreduce, c->d_enc_out, c->d_enc_out.cap,
                                    out->cell_off, &total)) != DGREP_OK) {
      dgrep_batch_partitions_free(out);
      return rc;
    }
    if (total <= c->d_enc_out.cap) break;
    if ((rc = grow(c, c->d_enc_out, total + total / 16)) != DGREP_OK) {
      dgrep_batch_partitions_free(out);
      return rc;
    }
  }
  out->nsplits = nsplits;
  out->nreduce = nreduce;
  out->total = total;
  if (total) {
    out->bytes = static_cast<uint8_t*>(malloc(total));
    if (!out->bytes) { dgrep_batch_partitions_free(out); return DGREP_E_NOMEM; }
    HIPCHK(hipMemcpyAsync(out->bytes, c->d_enc_out, total, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
  }
  return DGREP_OK;
}

extern "C" void dgrep_batch_partitions_free(dgrep_batch_partitions* p) {
  if (!p) return;
  free(p->cell_off);
  free(p->bytes);
  memset(p, 0, sizeof *p);
}

// ---- reduce task (map_reduce/worker.go:22-68,161-165 + grep.go:38-40) -------
extern "C" int dgrep_reduce(dgrep_ctx* c, const uint8_t* data, size_t n, dgrep_reduce_out* out) {
  if (!c || !out || (n && !data)) return DGREP_E_INVALID;
  memset(out, 0, sizeof *out);
  HIPCHK(hipSetDevice(c->device));
  if (n == 0) return DGREP_OK;
  int rc;
  if ((rc = grow(c, c->d_data, (n + 63) & ~uint64_t(63))) != DGREP_OK) return rc;
  if ((rc = ingest_resident(c, &data, &n, 1, n)) != DGREP_OK) return rc;
  uint64_t* d_info = reinterpret_cast<uint64_t*>(c->d_counters.p);  // 3 of its 4 u64
  HIPCHK(reduce_count_lines(c->d_data, n, d_info, c->stream));
  uint64_t nlines = 0;
  HIPCHK(hipMemcpyAsync(&nlines, d_info, 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  if (data[n - 1] != '\n') {
    c->err = "reduce input must be whole json.Encoder lines (the last byte is not '\\n')";
    return DGREP_E_INVALID;
  }
  size_t need = 0;
  HIPCHK(reduce_lines(c->d_data, n, nlines, nullptr, &need, nullptr, 0, d_info, c->stream));
  if ((rc = grow(c, c->d_red_scratch, need)) != DGREP_OK) return rc;
  uint64_t info[3] = {0, 0, 0};
  for (int attempt = 0; attempt < 2; ++attempt) {
    size_t have = c->d_red_scratch.cap;
    HIPCHK(hipEventRecord(c->ev0, c->stream));
    HIPCHK(reduce_lines(c->d_data, n, nlines, c->d_red_scratch, &have, c->d_red_out, c->d_red_out.cap, d_info,
                        c->stream));
    HIPCHK(hipEventRecord(c->ev1, c->stream));
    HIPCHK(hipMemcpyAsync(info, d_info, sizeof info, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (info[1] != UINT64_MAX) {
      c->err = "reduce input line " + std::to_string(info[1] + 1) + " is not a {\"Key\":\"..\",\"Value\":\"..\"} line";
      return DGREP_E_INVALID;
    }
    if (info[2] <= c->d_red_out.cap) break;
    if ((rc = grow(c, c->d_red_out, info[2])) != DGREP_OK) return rc;
  }
  HIPCHK(hipEventElapsedTime(&c->last_ms, c->ev0, c->ev1));
  out->lines_in = info[0];
  out->total = info[2];
  if (info[2]) {
    out->bytes = static_cast<uint8_t*>(malloc(info[2]));
    if (!out->bytes) return DGREP_E_NOMEM;
    HIPCHK(hipMemcpyAsync(out->bytes, c->d_red_out, info[2], hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
  }
  return DGREP_OK;
}

extern "C" void dgrep_reduce_free(dgrep_reduce_out* r) {
  if (!r) return;
  free(r->bytes);
  memset(r, 0, sizeof *r);
}

// ---- every reduce task of a job in one pass (kernels/reduce_batch.h) ---------
// Core of the batch reduce forms and of the job: data[0:n) is resident at
// d_data, the segment table (nseg + 1 u64) on the DEVICE at d_seg; nlines = the
// '\n' in data. One launch train into d_out, then the info words and the
// partition tables come back with one host wait. part_off (host, nparts + 1),
// lines_in (host, nparts, may be null); *total = the bytes needed.
static int reduce_batch_resident(dgrep_ctx* c, const uint8_t* d_data, uint64_t n, const uint64_t* d_seg, uint64_t nseg,
                                 uint32_t nparts, uint64_t nlines, uint8_t* d_out, uint64_t out_cap,
                                 uint64_t* part_off, uint64_t* lines_in, uint64_t* total) {
  *total = 0;
  if (nlines >= (uint64_t(1) << 32)) {
    c->err = "batch reduce: 2^32 or more lines";
    return DGREP_E_UNSUPPORTED;
  }
  if (n && (reinterpret_cast<uintptr_t>(d_data) & 15)) {
    c->err = "batch reduce: the device buffer must be 16-byte aligned";
    return DGREP_E_INVALID;
  }
  int rc;
  if ((rc = grow(c, c->d_rb_off, 2 * uint64_t(nparts) + 1)) != DGREP_OK) return rc;
  for (Event* e : {&c->evr0, &c->evr1}) HIPCHK(e->create());
  ReduceBatchArgs a;
  a.data = d_data;
  a.n = n;
  a.seg_off = d_seg;
  a.nseg = nseg;
  a.nparts = nparts;
  a.nlines = nlines;
  uint64_t* d_info = reinterpret_cast<uint64_t*>(c->d_counters.p);  // 3 of its u64
  uint64_t* d_part_off = c->d_rb_off;
  uint64_t* d_lines_in = c->d_rb_off + nparts + 1;
  size_t need = 0;
  HIPCHK(reduce_batch(a, nullptr, &need, nullptr, 0, nullptr, nullptr, d_info, c->stream));
  if ((rc = grow(c, c->d_red_scratch, need)) != DGREP_OK) return rc;
  size_t have = c->d_red_scratch.cap;
  uint64_t info[3] = {0, 0, 0};
  HIPCHK(hipEventRecord(c->evr0, c->stream));
  HIPCHK(reduce_batch(a, c->d_red_scratch, &have, d_out, out_cap, d_part_off, d_lines_in, d_info, c->stream));
  HIPCHK(hipEventRecord(c->evr1, c->stream));
  HIPCHK(hipMemcpyAsync(info, d_info, sizeof info, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipMemcpyAsync(part_off, d_part_off, (uint64_t(nparts) + 1) * 8, hipMemcpyDeviceToHost, c->stream));
  if (lines_in) HIPCHK(hipMemcpyAsync(lines_in, d_lines_in, uint64_t(nparts) * 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  HIPCHK(hipEventElapsedTime(&c->last_reduce_ms, c->evr0, c->evr1));
  if (info[1] != UINT64_MAX) {
    memset(part_off, 0, (uint64_t(nparts) + 1) * 8);
    if (lines_in) memset(lines_in, 0, uint64_t(nparts) * 8);
    c->err = "reduce input of partition " + std::to_string(reduce_batch_bad_part(info[1])) + ": line " +
             std::to_string(reduce_batch_bad_line(info[1]) + 1) +
             ((info[1] & 1) ? " is not a {\"Key\":\"..\",\"Value\":\"..\"} line"
                            : " is the unfinished last line of a segment (its last byte is not '\\n')");
    return DGREP_E_INVALID;
  }
  if (info[0] != nlines) {
    c->err = "batch reduce: the line count does not match the buffer";
    return DGREP_E_INVALID;
  }
  *total = info[2];
  return DGREP_OK;
}

// the '\n' in d_data[0:n): one kernel and one host wait
static int reduce_count_host(dgrep_ctx* c, const uint8_t* d_data, uint64_t n, uint64_t* nlines) {
  uint64_t* d_info = reinterpret_cast<uint64_t*>(c->d_counters.p);
  *nlines = 0;
  if (n == 0) return DGREP_OK;
  HIPCHK(reduce_count_lines(d_data, n, d_info, c->stream));
  HIPCHK(hipMemcpyAsync(nlines, d_info, 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return DGREP_OK;
}

// fills a reduce_batch_out from the context's output buffer (after its tables)
static int reduce_batch_fetch(dgrep_ctx* c, uint64_t total, dgrep_reduce_batch_out* out) {
  out->total = total;
  if (total) {
    out->bytes = static_cast<uint8_t*>(malloc(total));
    if (!out->bytes) return DGREP_E_NOMEM;
    HIPCHK(hipMemcpyAsync(out->bytes, c->d_red_out, total, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
  }
  return DGREP_OK;
}

// the pass into the context's output buffer, grown once if it was too small
static int reduce_batch_owned(dgrep_ctx* c, const uint8_t* d_data, uint64_t n, const uint64_t* d_seg, uint64_t nseg,
                              uint32_t nparts, uint64_t nlines, dgrep_reduce_batch_out* out) {
  int rc;
  uint64_t total = 0;
  for (int attempt = 0; attempt < 2; ++attempt) {
    if ((rc = reduce_batch_resident(c, d_data, n, d_seg, nseg, nparts, nlines, c->d_red_out, c->d_red_out.cap,
                                    out->part_off, out->lines_in, &total)) != DGREP_OK)
      return rc;
    if (total <= c->d_red_out.cap) break;
    if ((rc = grow(c, c->d_red_out, total)) != DGREP_OK) return rc;
  }
  return reduce_batch_fetch(c, total, out);
}

static bool reduce_batch_alloc(dgrep_reduce_batch_out* out, uint32_t nparts) {
  out->part_off = static_cast<uint64_t*>(calloc(size_t(nparts) + 1, 8));
  out->lines_in = static_cast<uint64_t*>(calloc(nparts, 8));
  if (!out->part_off || !out->lines_in) {
    dgrep_reduce_batch_free(out);
    return false;
  }
  out->nparts = nparts;
  return true;
}

extern "C" int dgrep_reduce_batch(dgrep_ctx* c, const uint8_t* const* data, const size_t* n, size_t nparts,
                                  dgrep_reduce_batch_out* out) {
  if (out) memset(out, 0, sizeof *out);
  if (!c || !out || !data || !n || nparts == 0 || nparts > kReduceBatchMaxParts) return DGREP_E_INVALID;
  size_t total_in = 0;
  for (size_t p = 0; p < nparts; ++p) {
    if (n[p] && !data[p]) return DGREP_E_INVALID;
    if (n[p] > ~size_t(0) - total_in) {
      c->err = "dgrep_reduce_batch: the input lengths overflow";
      return DGREP_E_INVALID;
    }
    total_in += n[p];
  }
  if (!reduce_batch_alloc(out, uint32_t(nparts))) return DGREP_E_NOMEM;
  if (total_in == 0) return DGREP_OK;  // nothing to read: every mr-out-<p> is empty
  auto fail = [&](int rc) {
    dgrep_reduce_batch_free(out);
    return rc;
  };
  if (hipError_t e = hipSetDevice(c->device); e != hipSuccess) return fail(hip_fail(c, e, "hipSetDevice"));
  int rc;
  if ((rc = grow(c, c->d_data, (uint64_t(total_in) + 63) & ~uint64_t(63))) != DGREP_OK) return fail(rc);
  if ((rc = ingest_resident(c, data, n, nparts, total_in, false)) != DGREP_OK) return fail(rc);
  std::vector<uint64_t> seg(nparts + 1, 0);
  for (size_t p = 0; p < nparts; ++p) seg[p + 1] = seg[p] + n[p];
  if ((rc = grow(c, c->d_rb_seg, nparts + 1)) != DGREP_OK) return fail(rc);
  if (hipError_t e = hipMemcpyAsync(c->d_rb_seg, seg.data(), (nparts + 1) * 8, hipMemcpyHostToDevice, c->stream);
      e != hipSuccess)
    return fail(hip_fail(c, e, "hipMemcpyAsync"));
  uint64_t nlines = 0;
  if ((rc = reduce_count_host(c, c->d_data, total_in, &nlines)) != DGREP_OK) return fail(rc);  // (waits: seg is uploaded)
  if ((rc = reduce_batch_owned(c, c->d_data, total_in, c->d_rb_seg, nparts, uint32_t(nparts), nlines, out)) != DGREP_OK)
    return fail(rc);
  return DGREP_OK;
}

extern "C" void dgrep_reduce_batch_free(dgrep_reduce_batch_out* r) {
  if (!r) return;
  free(r->part_off);
  free(r->lines_in);
  free(r->bytes);
  memset(r, 0, sizeof *r);
}

extern "C" int dgrep_reduce_batch_device(dgrep_ctx* c, const void* d_data, size_t n, const uint64_t* seg_off,
                                         size_t nseg, uint32_t nparts, void* d_out, uint64_t out_cap,
                                         uint64_t* part_off, uint64_t* lines_in, uint64_t* total) {
  if (total) *total = 0;
  if (!c || !total || !part_off || !seg_off || nseg == 0 || nparts == 0 || (n && !d_data) || (out_cap && !d_out))
    return DGREP_E_INVALID;
  // the limits come before seg_off is read
  if (nparts > kReduceBatchMaxParts) {
    c->err = "dgrep_reduce_batch_device: nparts must be at most 65535";
    return DGREP_E_UNSUPPORTED;
  }
  if (uint64_t(nseg) >= (uint64_t(1) << 32)) {
    c->err = "dgrep_reduce_batch_device: nseg must be below 2^32 segments";
    return DGREP_E_UNSUPPORTED;
  }
  if (nseg % nparts != 0) {
    c->err = "dgrep_reduce_batch_device: nseg must be a multiple of nparts";
    return DGREP_E_INVALID;
  }
  bool ok = seg_off[0] == 0 && seg_off[nseg] == n;
  for (size_t g = 0; ok && g < nseg; ++g) ok = seg_off[g] <= seg_off[g + 1];
  if (!ok) {
    c->err = "dgrep_reduce_batch_device: seg_off must ascend from 0 to n";
    return DGREP_E_INVALID;
  }
  if (n && (reinterpret_cast<uintptr_t>(d_data) & 15)) {
    c->err = "dgrep_reduce_batch_device: the device buffer must be 16-byte aligned";
    return DGREP_E_INVALID;
  }
  HIPCHK(hipSetDevice(c->device));
  int rc;
  if ((rc = grow(c, c->d_rb_seg, uint64_t(nseg) + 1)) != DGREP_OK) return rc;
  HIPCHK(hipMemcpyAsync(c->d_rb_seg, seg_off, (uint64_t(nseg) + 1) * 8, hipMemcpyHostToDevice, c->stream));
  uint64_t nlines = 0;
  if ((rc = reduce_count_host(c, static_cast<const uint8_t*>(d_data), n, &nlines)) != DGREP_OK) return rc;
  return reduce_batch_resident(c, static_cast<const uint8_t*>(d_data), n, c->d_rb_seg, nseg, nparts, nlines,
                               static_cast<uint8_t*>(d_out), out_cap, part_off, lines_in, total);
}

// ---- the whole grep job of one worker (worker.go:22-68,161-165 + grep.go) ----
extern "C" int dgrep_grep_job(dgrep_ctx* c, const uint8_t* const* data, const size_t* n, const char* const* filename,
                              const size_t* fn, size_t nsplits, uint32_t nreduce, dgrep_reduce_batch_out* out) {
  if (out) memset(out, 0, sizeof *out);
  if (!c || !out || !data || !n || nsplits == 0 || nsplits > UINT32_MAX) return DGREP_E_INVALID;
  int rc;
  if ((rc = encode_batch_args(c, filename, fn, nsplits, nreduce)) != DGREP_OK) return rc;
  for (size_t i = 0; i < nsplits; ++i)
    if (n[i] && !data[i]) return DGREP_E_INVALID;
  size_t total_in = 0;
  if (!pack_total(n, nsplits, &total_in) || total_in == ~size_t(0)) {
    c->err = "dgrep_grep_job: the split lengths overflow";
    return DGREP_E_INVALID;
  }
  if (uint64_t(nsplits) * nreduce >= (uint64_t(1) << 32)) {
    c->err = "dgrep_grep_job: nsplits * nreduce must be below 2^32 cells";
    return DGREP_E_UNSUPPORTED;
  }
  if (!c->loaded) { c->err = "no DFA loaded"; return DGREP_E_NO_DFA; }
  std::vector<uint8_t> names;
  if ((rc = build_name_table(c, filename, fn, nsplits, &names)) != DGREP_OK) return rc;
  HIPCHK(hipSetDevice(c->device));
  uint64_t count = 0;
  if ((rc = batch_scan_host(c, data, n, nsplits, total_in, false, &count)) != DGREP_OK) return rc;
  if (count >= (uint64_t(1) << 32)) { c->err = "more than 2^32-1 records"; return DGREP_E_UNSUPPORTED; }
  if (!reduce_batch_alloc(out, nreduce)) return DGREP_E_NOMEM;
  c->last_encode_ms = c->last_reduce_ms = 0.f;
  if (count == 0) return DGREP_OK;  // no matching line: every mr-out-<r> is empty
  auto fail = [&](int r) {
    dgrep_reduce_batch_free(out);
    return r;
  };
  // the cells stay in HBM: the encode's offsets are the reduce's segment table
  const uint64_t cells = uint64_t(nsplits) * nreduce;
  uint64_t enc_total = 0;
  for (int attempt = 0; attempt < 2; ++attempt) {
    if ((rc = encode_batch_resident(c, c->d_data, total_in, nsplits, c->d_res_line, c->d_res_start, c->d_res_len,
                                    c->d_res_split, count, names, nreduce, c->d_enc_out, c->d_enc_out.cap, nullptr,
                                    &enc_total)) != DGREP_OK)
      return fail(rc);
    if (enc_total <= c->d_enc_out.cap) break;
    if ((rc = grow(c, c->d_enc_out, enc_total + enc_total / 16)) != DGREP_OK) return fail(rc);
  }
  // one KeyValue line per record; the scratch is sized by the '\n' actually there
  uint64_t nlines = 0;
  if ((rc = reduce_count_host(c, c->d_enc_out, enc_total, &nlines)) != DGREP_OK) return fail(rc);
  if (nlines != count) {
    c->err = "dgrep_grep_job: the writer's output does not hold one line per record";
    return fail(DGREP_E_INVALID);
  }
  if ((rc = reduce_batch_owned(c, c->d_enc_out, enc_total, c->d_bat_cells, cells, nreduce, nlines, out)) != DGREP_OK)
    return fail(rc);
  return DGREP_OK;
}

// ---- the whole job in windows: files of any size (job_plan.h, kernels/job_arena.h)
// dgrep_grep_job with no input resident as a whole. Files arrive in task order;
// job_plan.h routes each one: small whole files are packed up to one window and
// flushed through the batch scan and the batch encode (the pack route), every
// other file streams through the job's one partition stream (the window
// route). Either way the encoded cells are appended on the device to the arena
// and their boundaries to the segment table, and dgrep_job_finish runs the batch
// reduce over both: segment g belongs to partition g % nreduce, and a
// partition's segments lie in task order, then line order.
struct dgrep_job {
  dgrep_ctx* c = nullptr;
  JobPlan plan;
  uint64_t gen = 0;
  int status = DGREP_OK;  // a failure mid-job: every later call returns it
  bool finished = false, in_file = false;
  dgrep_stream* s = nullptr;  // the window route: buffers, scratch and d_enc live as long as the job
  dgrep_encode_stats enc_sum = {};  // over the packs' encodes: dgrep_last_encode_stats after dgrep_job_finish
  // the open pack (host): P = f_0 '\n' f_1 ... as job_plan.h lays it out, and its files
  uint8_t* pack = nullptr;
  size_t pack_cap = 0;
  std::vector<size_t> pack_off, pack_len;
  std::vector<std::string> pack_name;
  // the arena and the segment table (device); plan.used bytes and plan.nseg + 1 entries are valid
  DevBuf<uint8_t> d_arena;
  uint64_t arena_growths = 0;
  DevBuf<uint64_t> d_seg;
  Event ev_a0, ev_a1;  // the last append
  bool append_untimed = false;
  float append_ms = 0.f, reduce_ms = 0.f;
};

// the last append's device time, once it is known to be done
static int job_append_ms_take(dgrep_job* j) {
  dgrep_ctx* c = j->c;
  if (!j->append_untimed) return DGREP_OK;
  HIPCHK(hipEventSynchronize(j->ev_a1));
  float ms = 0.f;
  HIPCHK(hipEventElapsedTime(&ms, j->ev_a0, j->ev_a1));
  j->append_ms += ms;
  j->append_untimed = false;
  return DGREP_OK;
}

// *p holds `need` units of T; the first `keep` survive. Old and new buffer
// exist together for the one device copy.
template <class T>
static int job_grow(dgrep_job* j, DevBuf<T>& b, uint64_t need, uint64_t keep, uint64_t initial, const char* what) {
  dgrep_ctx* c = j->c;
  if (b.holds(need)) return DGREP_OK;
  const uint64_t want = job_grow_cap(b.cap, need, initial);
  bool nomem = false;
  const hipError_t e = b.regrow(want, keep, c->stream, &nomem);  // (its wait: the copy, and every append into the old buffer)
  if (nomem) {
    c->err = std::string("job ") + what + ": out of device memory (" + std::to_string(want * sizeof(T)) + " bytes)";
    return DGREP_E_NOMEM;
  }
  HIPCHK(e);
  return DGREP_OK;
}

static int job_append_rows(dgrep_job* j, const uint8_t* d_src, uint64_t total, const uint64_t* d_end, uint64_t nend,
                           bool running_max, uint64_t rows, uint64_t lines) {
  dgrep_ctx* c = j->c;
  const uint64_t nseg0 = j->plan.nseg, used0 = j->plan.used;
  uint64_t at = 0;
  int limit = 0;
  if (!job_append(&j->plan, rows, total, lines, &at, &limit)) {
    c->err = limit == 0 ? "job: 2^32 or more segments (nreduce for every packed file and every window with a match)"
                        : "job: 2^32 or more matching lines";
    return DGREP_E_UNSUPPORTED;
  }
  int rc;
  const bool first = j->d_seg.p == nullptr;
  const uint64_t had = j->d_arena.cap;
  // (the reduce reads whole 16-byte vectors: the capacity is a multiple of 16)
  if ((rc = job_grow(j, j->d_arena, (at + total + 15) & ~uint64_t(15), used0, kJobArenaInitial,
                     "arena")) != DGREP_OK)
    return rc;
  if (had && j->d_arena.cap != had) ++j->arena_growths;
  if ((rc = job_grow(j, j->d_seg, j->plan.nseg + 1, nseg0 + 1, kJobSegInitial, "segment table")) !=
      DGREP_OK)
    return rc;
  if (first) HIPCHK(hipMemsetAsync(j->d_seg, 0, 8, c->stream));  // seg_off[0] = 0
  ArenaAppendArgs a;
  a.src = d_src;
  a.total = total;
  a.arena = j->d_arena;
  a.used = at;
  a.src_end = d_end;
  a.nend = nend;
  a.running_max = running_max;
  a.seg = j->d_seg + nseg0 + 1;
  if ((rc = job_append_ms_take(j)) != DGREP_OK) return rc;
  HIPCHK(hipEventRecord(j->ev_a0, c->stream));
  HIPCHK(arena_append(a, c->num_cus, c->stream));
  HIPCHK(hipEventRecord(j->ev_a1, c->stream));
  j->append_untimed = true;
  return DGREP_OK;
}

// The open pack through one packed ingest, one batch scan and one batch encode;
// its k * nreduce cells to the arena. A pack without a matching line appends
// nothing, as a window without one.
static int job_flush(dgrep_job* j) {
  dgrep_ctx* c = j->c;
  uint64_t bytes = 0;
  const uint64_t k = job_pack_flush(&j->plan, &bytes);
  if (k == 0 || (c->pat.flags & DGREP_DFA_MATCH_NONE)) return DGREP_OK;  // (no line can match: the plan's tallies only)
  std::vector<const uint8_t*> data(k);
  std::vector<const char*> fname(k);
  std::vector<size_t> fn(k);
  for (uint64_t i = 0; i < k; ++i) {
    data[i] = j->pack_len[i] ? j->pack + j->pack_off[i] : nullptr;
    fname[i] = j->pack_name[i].data();
    fn[i] = j->pack_name[i].size();
  }
  int rc;
  std::vector<uint8_t> names;
  if ((rc = build_name_table(c, fname.data(), fn.data(), k, &names)) != DGREP_OK) return rc;
  uint64_t count = 0;
  rc = batch_scan_host(c, data.data(), j->pack_len.data(), k, bytes, false, &count);
  j->pack_off.clear();
  j->pack_len.clear();
  j->pack_name.clear();
  if (rc != DGREP_OK) return rc;
  win_stats_add(j->s, bytes);
  if (count >= kJobMaxLines) { c->err = "job: 2^32 or more matching lines in one pack"; return DGREP_E_UNSUPPORTED; }
  if (count == 0) return DGREP_OK;
  uint64_t enc_total = 0;
  for (int attempt = 0; attempt < 2; ++attempt) {
    if ((rc = encode_batch_resident(c, c->d_data, bytes, k, c->d_res_line, c->d_res_start, c->d_res_len, c->d_res_split,
                                    count, names, j->plan.nreduce, c->d_enc_out, c->d_enc_out.cap, nullptr,
                                    &enc_total)) != DGREP_OK)
      return rc;
    j->s->call_encode_ms += c->last_encode_ms;
    // (the append kernel reads whole 16-byte vectors)
    if (enc_total <= c->d_enc_out.cap && ((enc_total + 15) & ~uint64_t(15)) <= c->d_enc_out.cap) break;
    if (attempt == 1) {
      c->err = "job: the pack's encoded size changed between two passes";
      return DGREP_E_HIP;
    }
    if ((rc = grow(c, c->d_enc_out, (enc_total + enc_total / 16 + 15) & ~uint64_t(15))) != DGREP_OK)
      return rc;
  }
  j->enc_sum.records += c->enc_stats.records;  // the pack's last attempt
  j->enc_sum.long_values += c->enc_stats.long_values;
  j->enc_sum.long_chunks += c->enc_stats.long_chunks;
  return job_append_rows(j, c->d_enc_out, enc_total, c->d_bat_cells + 1, k * uint64_t(j->plan.nreduce), false, k, count);
}

// the window route's next file: the stream's state is reset, its buffers stay
static int job_file_start(dgrep_job* j, const char* filename, size_t fn) {
  dgrep_ctx* c = j->c;
  dgrep_stream* s = j->s;
  const uint8_t* fname = reinterpret_cast<const uint8_t*>(filename);
  const uint64_t fj = json_escape_host(fname, fn, nullptr);
  if (fj >= (uint64_t(1) << 31)) { c->err = "filename too long"; return DGREP_E_INVALID; }
  std::vector<uint8_t> fjson(fj + 1);
  json_escape_host(fname, fn, fjson.data());
  int rc;
  if ((rc = grow(c, s->d_fname, fj + 1)) != DGREP_OK) return rc;
  HIPCHK(hipMemcpy(s->d_fname, fjson.data(), fj + 1, hipMemcpyHostToDevice));
  s->fname_json_len = uint32_t(fj);
  s->key_hash0 = key_prefix_hash(fname, fn);
  s->cur = 0;
  s->fill = 0;
  s->byte_base = s->line_base = 0;
  s->finished = false;
  return DGREP_OK;
}

// The checks every job call makes before it touches the GPU.
static int job_enter(dgrep_job* j, const char* call) {
  dgrep_ctx* c = j->c;
  if (j->status != DGREP_OK) return j->status;
  if (j->finished) {
    c->err = std::string(call) + " after dgrep_job_finish";
    return DGREP_E_INVALID;
  }
  if (j->gen != c->load_gen) {
    c->err = "a pattern was loaded while this job was open: its cells would mix two patterns";
    return DGREP_E_INVALID;
  }
  return DGREP_OK;
}

// a failure mid-job leaves the job unusable; nothing of the caller's is read after the return
static int job_fail(dgrep_job* j, int rc) {
  if (rc == DGREP_OK) return rc;
  dgrep_ctx* c = j->c;
  const std::string msg = c->err;
  j->status = rc;
  if (c->ing.copy_stream) (void)hipStreamSynchronize(c->ing.copy_stream);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  (void)hipGetLastError();
  c->err = msg;
  return rc;
}

extern "C" void dgrep_job_close(dgrep_job* j) {
  if (!j) return;
  dgrep_ctx* c = j->c;
  (void)hipSetDevice(c->device);
  if (j->s) dgrep_stream_close(j->s);  // (waits for both streams)
  else if (c->stream) (void)hipStreamSynchronize(c->stream);
  if (j->pack && !c->h_job_pack) {  // kept for the context's next job
    c->h_job_pack = j->pack;
    c->h_job_pack_cap = j->pack_cap;
  } else {
    free(j->pack);
  }
  delete j;
}

static int job_open(dgrep_ctx* c, size_t window_bytes, uint32_t nreduce, dgrep_job** out) {
  dgrep_job* j = new dgrep_job();
  j->c = c;
  j->plan.window = window_bytes;
  j->plan.nreduce = nreduce;
  j->gen = c->load_gen;
  *out = j;  // kept on failure too: dgrep_job_close frees what was made
  j->pack = c->h_job_pack;
  j->pack_cap = c->h_job_pack_cap;
  c->h_job_pack = nullptr;
  c->h_job_pack_cap = 0;
  int rc;
  if ((rc = win_open(c, window_bytes, 0, &j->s)) != DGREP_OK) return rc;
  dgrep_stream* s = j->s;
  s->parts = true;
  s->nreduce = nreduce;
  s->job = j;
  s->h_pbounds.assign(2 * size_t(nreduce) + 2, 0);
  if ((rc = grow(c, s->d_pbounds, s->h_pbounds.size())) != DGREP_OK) return rc;
  for (Event* e : {&s->ev_e0, &s->ev_e1, &j->ev_a0, &j->ev_a1}) HIPCHK(e->create());
  win_stats_begin(s);  // the scan stats and the encode time are summed over the job
  return DGREP_OK;
}

extern "C" int dgrep_job_open(dgrep_ctx* c, size_t window_bytes, uint32_t nreduce, dgrep_job** out) {
  if (out) *out = nullptr;
  if (!c || !out) return DGREP_E_INVALID;
  int rc;
  if ((rc = parts_args_ok(c, window_bytes, nullptr, 0, nreduce)) != DGREP_OK) return rc;
  HIPCHK(hipSetDevice(c->device));
  rc = job_open(c, window_bytes, nreduce, out);
  if (rc != DGREP_OK) {
    const std::string msg = c->err;
    dgrep_job_close(*out);
    c->err = msg;
    *out = nullptr;
  }
  return rc;
}

// the window route from its first byte: the pack goes first, so the arena stays in task order
static int job_window_begin(dgrep_job* j, const char* filename, size_t fn, bool flush_first) {
  int rc;
  if (flush_first && (rc = job_flush(j)) != DGREP_OK) return rc;
  return job_file_start(j, filename, fn);
}

extern "C" int dgrep_job_add(dgrep_job* j, const uint8_t* data, size_t n, const char* filename, size_t fn) {
  if (!j || (n && !data)) return DGREP_E_INVALID;
  dgrep_ctx* c = j->c;
  if (fn && !filename) { c->err = "filename is NULL with fn != 0"; return DGREP_E_INVALID; }
  int rc;
  if ((rc = job_enter(j, "dgrep_job_add")) != DGREP_OK) return rc;
  if (j->in_file) { c->err = "dgrep_job_add inside a file: dgrep_job_file_end comes first"; return DGREP_E_INVALID; }
  const JobStep step = job_next_file(&j->plan, n, false);
  if (c->pat.flags & DGREP_DFA_MATCH_NONE) {  // no line can match: the file is routed and counted, nothing is copied
    if (step.flush_first) (void)job_flush(j);
    if (step.route == kJobRoutePack) job_pack_push(&j->plan, n);
    return DGREP_OK;
  }
  HIPCHK(hipSetDevice(c->device));
  if (step.route == kJobRouteWindow) {
    if ((rc = job_fail(j, job_window_begin(j, filename, fn, step.flush_first))) != DGREP_OK) return rc;
    if ((rc = job_fail(j, win_feed(j->s, data, n))) != DGREP_OK) return rc;
    return job_fail(j, win_finish(j->s));
  }
  if (step.flush_first && (rc = job_fail(j, job_flush(j))) != DGREP_OK) return rc;
  // the caller's bytes are borrowed for this call only: the pack keeps a copy
  const uint64_t off = job_pack_push(&j->plan, n);
  if (off + n > j->pack_cap) {
    // geometric up to the window, which no pack exceeds
    const size_t cap = std::max<size_t>(off + n, std::min<size_t>(std::max<size_t>(2 * j->pack_cap, size_t(1) << 20),
                                                                   j->plan.window));
    uint8_t* p = static_cast<uint8_t*>(realloc(j->pack, cap));
    if (!p) { c->err = "job: out of host memory for the pack"; return job_fail(j, DGREP_E_NOMEM); }
    j->pack = p;
    j->pack_cap = cap;
  }
  if (off) j->pack[off - 1] = uint8_t('\n');
  pack_copy_threaded(j->pack + off, data, n, std::max(1, c->ing.threads));  // as the ingest copies a large piece
  j->pack_off.push_back(off);
  j->pack_len.push_back(n);
  j->pack_name.emplace_back(filename ? filename : "", fn);
  return DGREP_OK;
}

extern "C" int dgrep_job_file_begin(dgrep_job* j, const char* filename, size_t fn) {
  if (!j) return DGREP_E_INVALID;
  dgrep_ctx* c = j->c;
  if (fn && !filename) { c->err = "filename is NULL with fn != 0"; return DGREP_E_INVALID; }
  int rc;
  if ((rc = job_enter(j, "dgrep_job_file_begin")) != DGREP_OK) return rc;
  if (j->in_file) { c->err = "dgrep_job_file_begin inside a file: dgrep_job_file_end comes first"; return DGREP_E_INVALID; }
  j->in_file = true;
  const JobStep step = job_next_file(&j->plan, 0, true);
  if (c->pat.flags & DGREP_DFA_MATCH_NONE) {
    if (step.flush_first) (void)job_flush(j);
    return DGREP_OK;
  }
  HIPCHK(hipSetDevice(c->device));
  return job_fail(j, job_window_begin(j, filename, fn, step.flush_first));
}

extern "C" int dgrep_job_file_feed(dgrep_job* j, const uint8_t* data, size_t n) {
  if (!j || (n && !data)) return DGREP_E_INVALID;
  dgrep_ctx* c = j->c;
  int rc;
  if ((rc = job_enter(j, "dgrep_job_file_feed")) != DGREP_OK) return rc;
  if (!j->in_file) { c->err = "dgrep_job_file_feed without dgrep_job_file_begin"; return DGREP_E_INVALID; }
  if (n == 0 || (c->pat.flags & DGREP_DFA_MATCH_NONE)) return DGREP_OK;
  HIPCHK(hipSetDevice(c->device));
  return job_fail(j, win_feed(j->s, data, n));
}

extern "C" int dgrep_job_file_end(dgrep_job* j) {
  if (!j) return DGREP_E_INVALID;
  dgrep_ctx* c = j->c;
  int rc;
  if ((rc = job_enter(j, "dgrep_job_file_end")) != DGREP_OK) return rc;
  if (!j->in_file) { c->err = "dgrep_job_file_end without dgrep_job_file_begin"; return DGREP_E_INVALID; }
  j->in_file = false;
  if (c->pat.flags & DGREP_DFA_MATCH_NONE) return DGREP_OK;
  HIPCHK(hipSetDevice(c->device));
  return job_fail(j, win_finish(j->s));
}

static int job_finish(dgrep_job* j, dgrep_reduce_batch_out* out) {
  dgrep_ctx* c = j->c;
  int rc;
  if ((rc = job_flush(j)) != DGREP_OK) return rc;
  if ((rc = job_append_ms_take(j)) != DGREP_OK) return rc;
  win_stats_end(j->s);  // the sums over the job's packs and windows
  c->last_reduce_ms = 0.f;
  if (j->plan.lines == 0) return DGREP_OK;  // no matching line: every mr-out-<r> is empty
  // the table's last entry is the arena's end, or the appends and the plan disagree
  uint64_t end = 0;
  HIPCHK(hipMemcpyAsync(&end, j->d_seg + j->plan.nseg, 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  if (end != j->plan.used) {
    c->err = "dgrep_job_finish: the segment table does not end where the arena does";
    return DGREP_E_HIP;
  }
  uint64_t nlines = 0;
  if ((rc = reduce_count_host(c, j->d_arena, j->plan.used, &nlines)) != DGREP_OK) return rc;
  if (nlines != j->plan.lines) {
    c->err = "dgrep_job_finish: the arena does not hold one line per record";
    return DGREP_E_INVALID;
  }
  rc = reduce_batch_owned(c, j->d_arena, j->plan.used, j->d_seg, j->plan.nseg, j->plan.nreduce, nlines, out);
  j->reduce_ms = c->last_reduce_ms;
  return rc;
}

extern "C" int dgrep_job_finish(dgrep_job* j, dgrep_reduce_batch_out* out) {
  if (out) memset(out, 0, sizeof *out);
  if (!j || !out) return DGREP_E_INVALID;
  dgrep_ctx* c = j->c;
  int rc;
  if ((rc = job_enter(j, "dgrep_job_finish")) != DGREP_OK) return rc;
  if (j->in_file) { c->err = "dgrep_job_finish inside a file: dgrep_job_file_end comes first"; return DGREP_E_INVALID; }
  if (!reduce_batch_alloc(out, j->plan.nreduce)) return DGREP_E_NOMEM;
  HIPCHK(hipSetDevice(c->device));
  if ((rc = job_fail(j, job_finish(j, out))) != DGREP_OK) {
    const std::string msg = c->err;
    dgrep_reduce_batch_free(out);
    c->err = msg;
    return rc;
  }
  j->finished = true;
  c->enc_stats = j->enc_sum;  // the sums over the job's packs
  return DGREP_OK;
}

extern "C" int dgrep_job_stats_get(dgrep_job* j, dgrep_job_stats* out, size_t out_size) {
  if (!j || !out || out_size == 0) return DGREP_E_INVALID;
  dgrep_job_stats st;
  memset(&st, 0, sizeof st);
  const dgrep_stream* s = j->s;
  st.files = j->plan.files;
  st.packs = j->plan.packs;
  st.files_packed = j->plan.files_packed;
  st.files_windowed = j->plan.files_windowed;
  st.windows = s->windows;
  st.rows = j->plan.rows;
  st.segments = j->plan.nseg;
  st.arena_bytes = j->plan.used;
  st.arena_device_bytes = j->d_arena.cap;
  st.window_device_bytes = s->buf[0].cap + s->buf[1].cap;
  st.long_values = s->long_values;
  st.arena_growths = j->arena_growths;
  st.scan_ms = s->agg_ms;
  st.encode_ms = s->call_encode_ms;
  st.append_ms = j->append_ms;
  st.reduce_ms = j->reduce_ms;
  // a shorter (older) caller layout gets its own size; a longer one a zeroed tail
  const size_t k = std::min(out_size, sizeof st);
  memcpy(out, &st, k);
  if (out_size > k) memset(reinterpret_cast<uint8_t*>(out) + k, 0, out_size - k);
  return DGREP_OK;
}

extern "C" int dgrep_grep_job_windowed(dgrep_ctx* c, const uint8_t* const* data, const size_t* n,
                                       const char* const* filename, const size_t* fn, size_t nsplits, uint32_t nreduce,
                                       size_t window_bytes, dgrep_reduce_batch_out* out) {
  if (out) memset(out, 0, sizeof *out);
  if (!c || !out || (nsplits && (!data || !n || !filename || !fn))) return DGREP_E_INVALID;
  for (size_t i = 0; i < nsplits; ++i)
    if ((n[i] && !data[i]) || (fn[i] && !filename[i])) return DGREP_E_INVALID;
  dgrep_job* j = nullptr;
  int rc = dgrep_job_open(c, window_bytes, nreduce, &j);
  for (size_t i = 0; rc == DGREP_OK && i < nsplits; ++i) rc = dgrep_job_add(j, data[i], n[i], filename[i], fn[i]);
  if (rc == DGREP_OK) rc = dgrep_job_finish(j, out);
  const std::string msg = c->err;
  dgrep_job_close(j);  // the context holds no job when the call returns
  c->err = msg;
  return rc;
}

extern "C" int dgrep_last_reduce_ms(dgrep_ctx* c, float* ms) {
  if (!c || !ms) return DGREP_E_INVALID;
  *ms = c->last_reduce_ms;
  return DGREP_OK;
}

extern "C" int dgrep_last_encode_ms(dgrep_ctx* c, float* ms) {
  if (!c || !ms) return DGREP_E_INVALID;
  *ms = c->last_encode_ms;
  return DGREP_OK;
}

extern "C" int dgrep_last_encode_stats(dgrep_ctx* c, dgrep_encode_stats* out, size_t out_size) {
  if (!c || !out || out_size == 0) return DGREP_E_INVALID;
  dgrep_encode_stats st;
  memset(&st, 0, sizeof st);  // the padding behind encode_ms too
  st.records = c->enc_stats.records;
  st.long_values = c->enc_stats.long_values;
  st.long_chunks = c->enc_stats.long_chunks;
  st.encode_ms = c->last_encode_ms;
  // a shorter (older) caller layout gets its own size; a longer one a zeroed tail
  const size_t k = std::min(out_size, sizeof st);
  memcpy(out, &st, k);
  if (out_size > k) memset(reinterpret_cast<uint8_t*>(out) + k, 0, out_size - k);
  return DGREP_OK;
}

extern "C" void dgrep_result_free(dgrep_result* r) {
  if (!r) return;
  free(r->line_no);
  free(r->start);
  free(r->len);
  memset(r, 0, sizeof *r);
}

extern "C" int dgrep_last_kernel_ms(dgrep_ctx* c, float* ms) {
  if (!c || !ms) return DGREP_E_INVALID;
  *ms = c->last_ms;
  return DGREP_OK;
}

extern "C" int dgrep_take_kernel_ms(dgrep_ctx* c, double* sum_ms, uint64_t* scans) {
  if (!c || !sum_ms || !scans) return DGREP_E_INVALID;
  *sum_ms = c->ms_sum;
  *scans = c->ms_scans;
  c->ms_sum = 0.0;
  c->ms_scans = 0;
  return DGREP_OK;
}

extern "C" int dgrep_last_scan_stats(dgrep_ctx* c, dgrep_scan_stats* out, size_t out_size) {
  if (!c || !out || out_size == 0) return DGREP_E_INVALID;
  // a shorter (older) caller layout gets its own size; a longer one a zeroed tail
  const size_t k = std::min(out_size, sizeof(dgrep_scan_stats));
  memcpy(out, &c->stats, k);
  if (out_size > k) memset(reinterpret_cast<uint8_t*>(out) + k, 0, out_size - k);
  return DGREP_OK;
}


// ---- synthetic corpus ------------------------------------------------------
__global__ void synth_kernel(char* out, uint64_t n, uint64_t seed, int kind) {
  const uint64_t pages = (n + synth::kPage - 1) / synth::kPage;
  for (uint64_t p = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x; p < pages; p += uint64_t(gridDim.x) * blockDim.x) {
    const uint64_t off = p * synth::kPage;
    const uint32_t bytes = uint32_t(std::min<uint64_t>(synth::kPage, n - off));
    synth::page_fill(seed, p, kind, out + off, bytes);
  }
}

extern "C" int dgrep_synth_corpus(dgrep_ctx* c, void* d_out, size_t n, uint64_t seed, int kind) {
  if (!c || (n && !d_out)) return DGREP_E_INVALID;
  HIPCHK(hipSetDevice(c->device));
  if (n == 0) return DGREP_OK;
  const uint64_t pages = (n + synth::kPage - 1) / synth::kPage;
  const int block = 256;
  const int grid = int(std::min<uint64_t>((pages + block - 1) / block, 65536));
  hipLaunchKernelGGL(synth_kernel, dim3(grid), dim3(block), 0, c->stream, static_cast<char*>(d_out), uint64_t(n),
                     seed, kind);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(c->stream));
  return DGREP_OK;
}

// Host twin of dgrep_synth_corpus (same code path, synth.h): used by tests to
// regenerate any window of a device corpus on the CPU.
extern "C" int dgrep_synth_corpus_host(void* out, size_t n, uint64_t seed, int kind) {
  if (n && !out) return DGREP_E_INVALID;
  const uint64_t pages = (n + synth::kPage - 1) / synth::kPage;
  for (uint64_t p = 0; p < pages; ++p) {
    const uint64_t off = p * synth::kPage;
    const uint32_t bytes = uint32_t(std::min<uint64_t>(synth::kPage, n - off));
    synth::page_fill(seed, p, kind, static_cast<char*>(out) + off, bytes);
  }
  return DGREP_OK;
}

extern "C" int dgrep_synth_keyword(uint64_t seed, int i, char* out16) {
  if (!out16 || i < 0 || i >= synth::kKeywords) return -1;
  return synth::keyword(seed, i, out16);
}
