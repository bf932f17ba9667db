// job_plan_test.cpp — the windowed job's host arithmetic (csrc/runtime/
// job_plan.h) under AddressSanitizer + UBSan, on the CPU, as a program of its
// own (not loaded into Python):
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I distributed-grep_amd/csrc/runtime tests/job_c/job_plan_test.cpp -o job_plan_test
//   ./job_plan_test
//
// The planner is driven as the runtime drives it. The pack buffer is a heap
// buffer of exactly window_bytes, the arena and the segment table are heap
// buffers of exactly the capacity job_grow_cap gives, and an append's source
// is a heap buffer of its total rounded up to 16 -- so a file placed one byte
// too far, an arena offset past the capacity or a vector read past the source
// is a heap overflow the sanitizer reports. The append is done as the kernel
// does it (job_copy_split: bytewise head, 16-byte vectors funnel-shifted from
// two aligned source vectors, bytewise tail). Everything is compared with a
// plain restatement: packs by a greedy walk, the arena by concatenation.
// Exit status 0 and "job_plan OK" = pass.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <random>
#include <string>
#include <vector>

#include "job_plan.h"

using namespace dgrep;

static int failures = 0;
#define EXPECT(cond, ...)                 \
  do {                                    \
    if (!(cond)) {                        \
      fprintf(stderr, __VA_ARGS__);       \
      fprintf(stderr, " (%s)\n", #cond);  \
      ++failures;                         \
    }                                     \
  } while (0)

struct File {
  uint64_t n;
  bool streamed;
};

// the append kernel's copy on the host: src is 16-byte aligned and readable up to total rounded up to 16
static void copy_as_the_kernel(uint8_t* arena, uint64_t at, const uint8_t* src, uint64_t total) {
  const JobCopySplit s = job_copy_split(at, total);
  uint8_t* dst = arena + at;
  for (uint64_t i = 0; i < s.head; ++i) dst[i] = src[i];
  for (uint64_t j = 0; j < s.vecs; ++j) {
    uint8_t two[32];
    memcpy(two, src + 16 * j, 16);
    if (s.head) memcpy(two + 16, src + 16 * j + 16, 16);  // the second vector only when the shift needs it
    memcpy(dst + s.head + 16 * j, two + s.head, 16);
  }
  const uint64_t tail_at = s.head + 16 * s.vecs;
  for (uint64_t i = 0; i < s.tail; ++i) dst[tail_at + i] = src[tail_at + i];
}

struct Sim {
  JobPlan plan;
  uint8_t* pack = nullptr;  // exactly `window` bytes
  std::vector<uint64_t> pack_off, pack_len;
  uint8_t* arena = nullptr;
  uint64_t arena_cap = 0;
  uint64_t* seg = nullptr;
  uint64_t seg_cap = 0;
  std::string want_arena;
  std::vector<uint64_t> want_seg{0};
  std::vector<std::vector<uint64_t>> packs;  // the files of every flushed pack, by length
  std::mt19937 rng;

  Sim(uint64_t window, uint32_t nreduce, unsigned seed) : rng(seed) {
    plan.window = window;
    plan.nreduce = nreduce;
    pack = static_cast<uint8_t*>(malloc(window));
  }
  ~Sim() {
    free(pack);
    free(arena);
    free(seg);
  }

  // rows * nreduce cells with random sizes: `total` bytes, appended as the runtime appends them
  void append(uint64_t rows) {
    const uint64_t cells = rows * plan.nreduce;
    std::vector<uint64_t> end(cells);
    uint64_t total = 0, lines = 0;
    for (uint64_t c = 0; c < cells; ++c) {
      if (rng() % 3) total += rng() % 70 + 1, ++lines;
      end[c] = total;
    }
    uint8_t* src = static_cast<uint8_t*>(aligned_alloc(16, total ? (total + 15) & ~uint64_t(15) : 16));
    for (uint64_t i = 0; i < total; ++i) src[i] = uint8_t(rng());
    const uint64_t used0 = plan.used, nseg0 = plan.nseg;
    uint64_t at = ~uint64_t(0);
    int limit = -1;
    const bool ok = job_append(&plan, rows, total, lines, &at, &limit);
    EXPECT(ok && at == used0 && plan.used == used0 + total && plan.nseg == nseg0 + cells, "append bookkeeping");
    // grow with the contents kept: old and new exist together for the one copy
    const uint64_t need = (at + total + 15) & ~uint64_t(15);
    const uint64_t cap = job_grow_cap(arena ? arena_cap : 0, need, kJobArenaInitial);
    EXPECT(cap >= need && (cap == arena_cap || cap >= 2 * arena_cap || arena_cap == 0), "arena growth");
    if (cap > kJobArenaInitial) EXPECT(cap < 2 * (at + total) + 32, "arena below twice what is used (%zu for %zu)",
                                       size_t(cap), size_t(at + total));
    if (cap != arena_cap || !arena) {
      uint8_t* fresh = static_cast<uint8_t*>(aligned_alloc(16, cap));
      if (used0) memcpy(fresh, arena, used0);
      free(arena);
      arena = fresh;
      arena_cap = cap;
    }
    const uint64_t scap = job_grow_cap(seg ? seg_cap : 0, plan.nseg + 1, kJobSegInitial);
    if (scap != seg_cap || !seg) {
      uint64_t* fresh = static_cast<uint64_t*>(malloc(scap * 8));
      if (seg) memcpy(fresh, seg, (nseg0 + 1) * 8);
      else fresh[0] = 0;
      free(seg);
      seg = fresh;
      seg_cap = scap;
    }
    copy_as_the_kernel(arena, at, src, total);
    for (uint64_t c = 0; c < cells; ++c) seg[nseg0 + 1 + c] = at + end[c];
    want_arena.append(reinterpret_cast<char*>(src), total);
    for (uint64_t c = 0; c < cells; ++c) want_seg.push_back(used0 + end[c]);
    free(src);
  }

  void flush() {
    uint64_t bytes = 0;
    const uint64_t k = job_pack_flush(&plan, &bytes);
    if (!k) return;
    EXPECT(k == pack_len.size() && bytes <= plan.window, "flush of %zu files, %zu bytes", size_t(k), size_t(bytes));
    uint64_t sum = k - 1;
    for (uint64_t n : pack_len) sum += n;
    EXPECT(sum == bytes, "pack bytes");
    // P as the ingest lays it out: every separator is where the plan left room for it
    for (uint64_t i = 1; i < k; ++i) EXPECT(pack[pack_off[i] - 1] == '\n', "separator before file %zu", size_t(i));
    packs.push_back(pack_len);
    pack_off.clear();
    pack_len.clear();
    if (rng() % 4) append(k);  // (a pack without a matching line appends nothing)
  }

  void add(const File& f) {
    const JobStep step = job_next_file(&plan, f.n, f.streamed);
    EXPECT(step.route == ((f.streamed || f.n > plan.window) ? kJobRouteWindow : kJobRoutePack), "route");
    if (step.route == kJobRouteWindow) {
      EXPECT(step.flush_first == !pack_len.empty(), "the pack goes before a windowed file");
      if (step.flush_first) flush();
      for (unsigned w = rng() % 4; w > 0; --w) append(1);  // the windows that completed a matching line
      return;
    }
    if (step.flush_first) flush();
    const uint64_t off = job_pack_push(&plan, f.n);
    if (off) pack[off - 1] = '\n';
    if (f.n) memset(pack + off, 'a' + int(pack_len.size() % 26), f.n);  // past `window` bytes: a heap overflow
    pack_off.push_back(off);
    pack_len.push_back(f.n);
  }
};

static void run(uint64_t window, uint32_t nreduce, const std::vector<File>& files, unsigned seed, const char* what) {
  Sim s(window, nreduce, seed);
  for (const File& f : files) s.add(f);
  s.flush();
  // the packs, restated: greedy in task order, cut by every windowed file
  std::vector<std::vector<uint64_t>> want;
  std::vector<uint64_t> cur;
  uint64_t bytes = 0, packed = 0, windowed = 0;
  for (const File& f : files) {
    if (f.streamed || f.n > window) {
      if (!cur.empty()) want.push_back(cur);
      cur.clear();
      bytes = 0;
      ++windowed;
      continue;
    }
    ++packed;
    if (!cur.empty() && bytes + 1 + f.n > window) {
      want.push_back(cur);
      cur.clear();
      bytes = 0;
    }
    bytes = cur.empty() ? f.n : bytes + 1 + f.n;
    cur.push_back(f.n);
  }
  if (!cur.empty()) want.push_back(cur);
  EXPECT(s.packs == want, "%s: the packs differ from the greedy walk", what);
  EXPECT(s.plan.files == files.size() && s.plan.files_packed == packed && s.plan.files_windowed == windowed &&
             s.plan.packs == want.size(),
         "%s: tallies", what);
  EXPECT(s.plan.used == s.want_arena.size() && s.plan.nseg + 1 == s.want_seg.size() && s.plan.nseg % nreduce == 0,
         "%s: totals", what);
  EXPECT(s.plan.used == 0 || memcmp(s.arena, s.want_arena.data(), s.plan.used) == 0, "%s: arena bytes", what);
  EXPECT(s.seg == nullptr || memcmp(s.seg, s.want_seg.data(), s.want_seg.size() * 8) == 0, "%s: segment table", what);
  for (size_t g = 0; g + 1 < s.want_seg.size(); ++g) EXPECT(s.want_seg[g] <= s.want_seg[g + 1], "%s: ascending", what);
}

int main() {
  const uint64_t W = 4096;
  // the route edge, a pack full to the byte, one that overflows by one, a windowed file between two packs
  run(W, 10, {{W, false}, {W - 1, false}, {W + 1, false}}, 1, "route edge");
  run(W, 10, {{2048, false}, {2047, false}, {300, false}}, 2, "full to the byte");
  run(W, 10, {{2048, false}, {2048, false}, {300, false}}, 3, "overflow by one");
  run(W, 10, {{500, false}, {600, false}, {3 * W, false}, {400, false}, {16, false}}, 4, "window between packs");
  run(W, 1, {{0, false}, {0, true}, {0, false}, {0, false}, {1, true}}, 5, "empty files");
  run(W, 10, {}, 6, "no file");
  run(W, 1000, {{10, false}, {W + 100, false}, {10, false}}, 7, "more segments than lines");
  std::vector<File> many(64, File{1024, false});
  run(65536, 10, many, 8, "64 x 1 KiB");
  std::mt19937 rng(2025);
  int lists = 9;
  for (int l = 0; l < 40; ++l, ++lists) {
    const uint64_t w = 4096u << (rng() % 3);
    std::vector<File> files(rng() % 60 + 1);
    for (File& f : files) {
      const unsigned kind = rng() % 10;
      f.n = kind < 5 ? rng() % 200 : kind < 8 ? rng() % (w + 1) : kind == 8 ? w + rng() % 3 - 1 : w + rng() % (3 * w);
      f.streamed = rng() % 4 == 0;
    }
    run(w, uint32_t(rng() % 12 + 1), files, 100 + l, "random");
  }
  // every head and tail length of the append's split, at every arena alignment
  for (uint64_t at = 0; at < 16; ++at)
    for (uint64_t total = 0; total < 80; ++total) {
      const JobCopySplit s = job_copy_split(at, total);
      EXPECT(s.head + 16 * s.vecs + s.tail == total && s.head < 16 && s.tail < 16 && ((at + s.head) % 16 == 0 || s.vecs == 0),
             "split at %zu total %zu", size_t(at), size_t(total));
    }
  // the limits: segments and lines stay below 2^32, and a refusal changes nothing
  JobPlan p;
  p.window = W;
  p.nreduce = 65535;
  uint64_t at = 0;
  int limit = -1;
  EXPECT(job_append(&p, 65536, 10, 5, &at, &limit) && p.nseg == uint64_t(65536) * 65535, "a large append");
  EXPECT(!job_append(&p, 2, 10, 5, &at, &limit) && limit == 0 && p.nseg == uint64_t(65536) * 65535 && p.used == 10,
         "2^32 segments refused");
  p.nreduce = 1;
  p.nseg = 0;
  EXPECT(job_append(&p, 1, 10, kJobMaxLines - 6, &at, &limit), "lines up to the limit");
  EXPECT(!job_append(&p, 1, 10, 1, &at, &limit) && limit == 1 && p.lines == kJobMaxLines - 1, "2^32 lines refused");
  // a pack never holds 2^32 cells
  JobPlan q;
  q.window = uint64_t(1) << 40;
  q.nreduce = 65535;
  q.pack_files = 65537;
  q.pack_bytes = 65536;
  EXPECT(!job_pack_fits(q, 0), "a pack of 2^32 cells refused");
  q.pack_files = 65536;  // 65537 * 65535 = 2^32 - 1 cells
  EXPECT(job_pack_fits(q, 0), "one file fewer fits");
  if (failures) return 1;
  printf("job_plan OK (%d file lists)\n", lists);
  return 0;
}
