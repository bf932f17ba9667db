// pattern_image_test.cpp -- stand-alone driver for the host-only pattern image
// builder (csrc/runtime/pattern_image.h), built with
// -fsanitize=address,undefined by tests/pattern_image_c/Makefile and linked
// with the pattern compiler, so it compiles its patterns itself. No HIP.
//
//   pattern_image_test [print | print-auto | check-print] [patterns file]
//
// The patterns (tests/golden/pattern_image_patterns.txt): the stepper cells,
// the bench configs' patterns, partial builds and a list of small patterns,
// each with a line that matches. Each is built under every stepper choice
// dgrep_set_stepper can ask for (kForces).
//
// Default mode: every image that builds is walked on the CPU by a one-lane
// restatement of its stepper's rule over a small corpus (twice: the corpus and
// the corpus less its first byte, so every '\n' falls on both parities), and
// the matching line numbers must equal a direct walk of the blob's trans /
// byte_class; the default-row image must reproduce every entry of `full`,
// st2id must name the blob state of every stepper state, the seeds must be
// live states. Refusals must carry dgrep_load_dfa's codes and messages.
// Prints "pattern_image OK <n>".
//
// print mode: one line per (pattern, force) with the image's scalars and a
// CRC-32 of each buffer (tests/golden/pattern_images.txt). check-print does
// both in one pass over the patterns (the test suite pays for the builds once);
// print-auto prints the unforced choice alone (a patterns file of the caller's).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "pattern_image.h"

using namespace dgrep;

#ifndef PATTERNS_FILE
#define PATTERNS_FILE "../golden/pattern_image_patterns.txt"
#endif

namespace {

struct Force {
  int force;
  uint32_t cap;  // 0: none
};
const Force kForces[] = {{0, 0}, {2, 0}, {3, 0}, {4, 0}, {4, 3}, {4, 4}, {4, 64}, {0, 3}};

const char kMsgBlob[] = "dgrep_load_dfa: malformed blob";
const char kMsgPartial[] =
    "dgrep_load_dfa: a partial DFA (over the compiler's state budget) runs on the filter stepper only";
const char kMsgPair[] = "dgrep_load_dfa: the pair stepper's two-byte table does not fit this DFA";
const char kMsgFilter[] = "dgrep_load_dfa: the filter stepper cannot hold this DFA's first states";

int g_fail = 0;
#define CHECK(cond, ...)                          \
  do {                                            \
    if (!(cond)) {                                \
      fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); \
      fprintf(stderr, __VA_ARGS__);               \
      fprintf(stderr, "\n");                      \
      ++g_fail;                                   \
      return;                                     \
    }                                             \
  } while (0)

uint32_t crc32(const void* p, size_t n) {
  static uint32_t tab[256];
  if (!tab[1])
    for (uint32_t i = 0; i < 256; ++i) {
      uint32_t c = i;
      for (int k = 0; k < 8; ++k) c = (c >> 1) ^ (0xedb88320u & (0u - (c & 1u)));
      tab[i] = c;
    }
  uint32_t c = 0xffffffffu;
  const uint8_t* b = static_cast<const uint8_t*>(p);
  for (size_t i = 0; i < n; ++i) c = tab[(c ^ b[i]) & 0xffu] ^ (c >> 8);
  return c ^ 0xffffffffu;
}
template <class V>
uint32_t crc_of(const std::vector<V>& v) {
  return crc32(v.data(), v.size() * sizeof(V));
}

struct Pattern {
  std::string name, hit, text;
  uint32_t budget = 0;
};

std::vector<Pattern> read_patterns(const char* path) {
  std::vector<Pattern> out;
  std::ifstream f(path);
  std::string line;
  while (std::getline(f, line)) {
    if (line.empty() || line[0] == '#') continue;
    const size_t a = line.find('\t'), b = line.find('\t', a + 1), c = line.find('\t', b + 1);
    if (a == std::string::npos || b == std::string::npos || c == std::string::npos) {
      fprintf(stderr, "bad line in %s: %s\n", path, line.c_str());
      exit(2);
    }
    Pattern p;
    p.name = line.substr(0, a);
    p.budget = uint32_t(strtoul(line.substr(a + 1, b - a - 1).c_str(), nullptr, 10));
    p.hit = line.substr(b + 1, c - b - 1);
    p.text = line.substr(c + 1);
    out.push_back(p);
  }
  return out;
}

// the blob as the builder gets it: an exact-size heap block
struct Blob {
  void* p = nullptr;
  size_t n = 0;
  dgrep_blob_header h;
  const uint32_t* trans() const {
    return reinterpret_cast<const uint32_t*>(static_cast<const uint8_t*>(p) + sizeof h);
  }
};

// Under 16 KiB, deterministic: lines with the hit at their start, middle and
// end, the hit alone, its prefixes, a damaged hit, filler, empty lines (so
// "\n\n" too); no '\n' at the end, the last line being the hit.
std::vector<uint8_t> make_corpus(const std::string& hit) {
  std::vector<uint8_t> d;
  uint32_t r = 12345u + uint32_t(hit.size());
  auto rnd = [&](uint32_t m) {
    r = r * 1664525u + 1013904223u;
    return (r >> 8) % m;
  };
  const std::string alpha = "abexy k019-_WARN:" + hit;
  auto filler = [&](uint32_t n) {
    for (uint32_t i = 0; i < n; ++i) d.push_back(uint8_t(alpha[rnd(uint32_t(alpha.size()))]));
  };
  auto put = [&](const std::string& s) { d.insert(d.end(), s.begin(), s.end()); };
  const size_t limit = 15 * 1024 - 2 * hit.size() - 64;
  while (d.size() < limit) {
    switch (rnd(9)) {
      case 0: put(hit); break;
      case 1: filler(rnd(40)); put(hit); break;
      case 2: put(hit); filler(rnd(40)); break;
      case 3: filler(rnd(20)); put(hit); filler(rnd(20)); break;
      case 4: filler(rnd(60)); break;
      case 5: break;  // an empty line
      case 6: put(hit.substr(0, hit.empty() ? 0 : rnd(uint32_t(hit.size())))); break;
      case 7: {
        std::string s = hit;
        if (!s.empty()) s[rnd(uint32_t(s.size()))] = '#';
        put(s);
        break;
      }
      default: filler(1 + rnd(3)); break;
    }
    d.push_back('\n');
  }
  put(hit);
  return d;
}

// ---- the walks: matching 1-based line numbers of strings.Split(data, "\n") ----
// (every walk ends with the '\n' the split's end stands for)

// what a line is on the blob itself; cand[i] = line i + 1 entered `cand_state`
std::vector<uint32_t> walk_blob(const Blob& b, const std::vector<uint8_t>& d, uint32_t cand_state,
                                std::vector<uint8_t>* cand) {
  const uint32_t K = b.h.nclasses;
  const uint32_t* T = b.trans();
  std::vector<uint32_t> out;
  uint32_t s = b.h.start, line = 1;
  bool in_cand = false;
  for (size_t i = 0; i <= d.size(); ++i) {
    const uint8_t c = i < d.size() ? d[i] : uint8_t('\n');
    s = T[size_t(s) * K + b.h.byte_class[c]];
    if (s == cand_state) in_cand = true;
    if (c == '\n') {
      if (s == b.h.start_m) out.push_back(line);
      if (cand) cand->push_back(in_cand);
      in_cand = false;
      ++line;
    }
  }
  return out;
}

// the blob state a stepper state stands for must follow the blob's own walk
struct Shadow {
  const Blob* b;
  const PatternImage* im;
  uint32_t s;
  bool on;
  Shadow(const Blob& bl, const PatternImage& i) : b(&bl), im(&i), s(bl.h.start), on(!i.st2id.empty()) {}
  void step(uint8_t c) { s = b->trans()[size_t(s) * b->h.nclasses + b->h.byte_class[c]]; }
  bool agrees(uint32_t stepper_index) const {
    return !on || (stepper_index < im->st2id.size() && im->st2id[stepper_index] == s);
  }
};

bool walk_sheng(const Blob& b, const PatternImage& im, const std::vector<uint8_t>& d, std::vector<uint32_t>* out) {
  if (im.table.size() != 256 * 8 || im.start % 0x01010101u || im.start_m != im.nstates - 1) return false;
  Shadow sh(b, im);
  uint32_t w = im.start, line = 1;  // the state replicated in the word's four bytes
  for (size_t i = 0; i <= d.size(); ++i) {
    const uint8_t c = i < d.size() ? d[i] : uint8_t('\n');
    w = im.table[size_t(c) * 8 + (w & 0xffu)] * 0x01010101u;
    sh.step(c);
    if ((w & 0xffu) >= im.nstates || !sh.agrees(w & 0xffu)) return false;
    if (c == '\n') {
      if ((w & 0xffu) == im.start_m) out->push_back(line);
      ++line;
    }
  }
  uint32_t lo = 0, hi = 0;
  for (int k = 0; k < 4; ++k) {
    lo |= uint32_t(im.table[size_t('\n') * 8 + k]) << (8 * k);
    hi |= uint32_t(im.table[size_t('\n') * 8 + 4 + k]) << (8 * k);
  }
  return lo == im.sheng_nl_lo && hi == im.sheng_nl_hi;
}

bool walk_table(const Blob& b, const PatternImage& im, const std::vector<uint8_t>& d, std::vector<uint32_t>* out) {
  if (im.table.size() != ((size_t(im.nstates) * kTableRow + 15) & ~size_t(15))) return false;
  Shadow sh(b, im);
  uint32_t s = im.start, line = 1;
  for (size_t i = 0; i <= d.size(); ++i) {
    const uint8_t c = i < d.size() ? d[i] : uint8_t('\n');
    s = im.table[size_t(s) * kTableRow + c];
    sh.step(c);
    if (s >= im.nstates || !sh.agrees(s)) return false;
    if (c == '\n') {
      if (s == im.start_m) out->push_back(line);
      ++line;
    }
  }
  return true;
}

// StepPair: T2 on two bytes (a pair ending at >= thr other than start_m: its
// first byte closed a matching line; at >= start_m: its second did), T1 on the
// odd last byte and on the split's end
bool walk_pair(const Blob& b, const PatternImage& im, const std::vector<uint8_t>& d, std::vector<uint32_t>* out) {
  const uint8_t* img = im.table.data();
  const size_t nb = im.table.size();
  const PairArgs& pa = im.pair_args;
  const uint32_t esz = pa.w32 ? 4 : 2, K = im.nclasses, M = im.start_m;
  if (nb > kPairMaxImage || pa.t1 >= nb || pa.div == 0) return false;
  auto index = [&](uint32_t v) { return (v - kPairT2) / pa.div; };
  auto t1 = [&](uint32_t v, uint8_t c, uint32_t* to) {
    const size_t at = pa.t1 + 2 * (size_t(index(v)) * K + img[c] / esz);
    if (v < kPairT2 || (v - kPairT2) % pa.div || at + 2 > nb) return false;
    uint16_t x;
    memcpy(&x, img + at, 2);
    *to = x;
    return true;
  };
  Shadow sh(b, im);
  uint32_t v = im.start, line = 1;
  const size_t n2 = d.size() & ~size_t(1);
  for (size_t i = 0; i < n2; i += 2) {
    uint16_t ck;
    memcpy(&ck, img + kPairCK + 2 * d[i], 2);
    const size_t at = size_t(v) + ck + img[d[i + 1]];
    if (v < kPairT2 || at + esz > pa.t1) return false;
    if (esz == 4) {
      memcpy(&v, img + at, 4);
    } else {
      uint16_t x;
      memcpy(&x, img + at, 2);
      v = x;
    }
    sh.step(d[i]);
    sh.step(d[i + 1]);
    if (v < kPairT2 || (v - kPairT2) % pa.div || !sh.agrees(index(v))) return false;
    const bool e1 = v >= pa.thr && v != M, e2 = v >= M;
    if (e1 && d[i] != '\n') return false;
    if (e2 && d[i + 1] != '\n') return false;
    if (e1) out->push_back(line);
    if (d[i] == '\n') ++line;
    if (e2) out->push_back(line);
    if (d[i + 1] == '\n') ++line;
  }
  for (size_t i = n2; i <= d.size(); ++i) {
    const uint8_t c = i < d.size() ? d[i] : uint8_t('\n');
    if (!t1(v, c, &v)) return false;
    sh.step(c);
    if (!sh.agrees(index(v))) return false;
    if (c == '\n') {
      if (v == M) out->push_back(line);
      ++line;
    }
  }
  return true;
}

// the whole DFA as verify_kernel reads it: one line from blob_start
bool full_line_matches(const Blob& b, const PatternImage& im, const uint8_t* p, size_t n) {
  const uint32_t K = b.h.nclasses;
  auto next = [&](uint32_t s, uint32_t k) {
    return im.full_u32 ? reinterpret_cast<const uint32_t*>(im.full.data())[size_t(s) * K + k]
                       : uint32_t(reinterpret_cast<const uint16_t*>(im.full.data())[size_t(s) * K + k]);
  };
  uint32_t s = im.blob_start;
  for (size_t i = 0; i < n && s != im.blob_matched; ++i) s = next(s, im.h_cls[p[i]]);
  return s == im.blob_matched || next(s, im.h_cls[uint8_t('\n')]) == im.blob_start_m;
}

// StepFilter: u16 rows after the class bytes, states premultiplied by the row
// pitch; a '\n' that enters a state >= start_m is an event, CAND_END a candidate
// (re-decided on `full`; with a partial blob's NFA program left a candidate)
bool walk_filter(const Blob& b, const PatternImage& im, const std::vector<uint8_t>& d, std::vector<uint32_t>* out,
                 std::vector<uint8_t>* cand) {
  const uint8_t* img = im.table.data();
  const size_t nb = im.table.size();
  if (nb > kFilterImageBytes || nb < kFilterClassBytes) return false;
  const bool partial = (im.flags & DGREP_DFA_PARTIAL) != 0;
  uint32_t s = im.start, line = 1;
  size_t line_start = 0;
  for (size_t i = 0; i <= d.size(); ++i) {
    const uint8_t c = i < d.size() ? d[i] : uint8_t('\n');
    const size_t at = kFilterClassBytes + 2 * (size_t(s) + img[c]);
    if (at + 2 > nb) return false;
    uint16_t x;
    memcpy(&x, img + at, 2);
    s = x;
    if (c == '\n') {
      bool is_cand = false;
      if (s >= im.start_m) {
        if (s != im.cand_end) out->push_back(line);
        else if (partial) is_cand = true;
        else if (full_line_matches(b, im, d.data() + line_start, i - line_start)) out->push_back(line);
      }
      cand->push_back(is_cand);
      ++line;
      line_start = i + 1;
    }
  }
  return true;
}

// ---- the passes after the scan ------------------------------------------------
void check_full(const Blob& b, const PatternImage& im, const char* what) {
  const uint32_t S = b.h.nstates, K = b.h.nclasses;
  CHECK(im.full.size() == size_t(S) * K * (im.full_u32 ? 4 : 2) && im.full_u32 == (S > 65535), "%s: full size", what);
  CHECK(im.blob_start < S && im.blob_start_m < S, "%s: blob_start", what);
  CHECK(im.verify_hot % K == 0 && im.verify_hot <= size_t(S) * K, "%s: verify_hot", what);
  CHECK(memcmp(im.h_cls, b.h.byte_class, 256) == 0, "%s: cls", what);
  auto full = [&](uint32_t s, uint32_t k) {
    return im.full_u32 ? reinterpret_cast<const uint32_t*>(im.full.data())[size_t(s) * K + k]
                       : uint32_t(reinterpret_cast<const uint16_t*>(im.full.data())[size_t(s) * K + k]);
  };
  // `full` is the blob's DFA under a renumbering: found by walking both from start and start_m
  std::vector<uint32_t> to(S, UINT32_MAX), queue;
  auto pair_up = [&](uint32_t x, uint32_t y) {
    if (to[x] == UINT32_MAX) { to[x] = y; queue.push_back(x); }
    return to[x] == y;
  };
  CHECK(pair_up(b.h.start, im.blob_start) && pair_up(b.h.start_m, im.blob_start_m), "%s: start ids", what);
  for (size_t q = 0; q < queue.size(); ++q)
    for (uint32_t k = 0; k < K; ++k) {
      const uint32_t y = full(to[queue[q]], k);
      CHECK(y < S && pair_up(b.trans()[size_t(queue[q]) * K + k], y), "%s: full is not the blob's DFA", what);
    }
  // the absorbing states
  const uint32_t cn = b.h.byte_class[uint8_t('\n')];
  for (uint32_t a : {im.blob_matched, im.blob_dead}) {
    if (a == UINT32_MAX) continue;
    CHECK(a < S, "%s: absorbing id", what);
    for (uint32_t k = 0; k < K; ++k)
      CHECK(full(a, k) == (k != cn ? a : a == im.blob_matched ? im.blob_start_m : im.blob_start),
            "%s: state %u is not absorbing", what, a);
  }
  // the seeds: live states
  CHECK(im.long_seed.size() == size_t(kLongSeeds) && im.long_seed[0] == im.blob_start, "%s: seeds", what);
  for (size_t i = 0; i < im.long_seed.size(); ++i) {
    const uint32_t x = im.long_seed[i];
    CHECK(x < S, "%s: seed %zu out of range", what, i);
    CHECK(x == im.blob_start || (x != im.blob_matched && x != im.blob_dead), "%s: seed %zu is absorbing", what, i);
  }
  // the default-row image gives every entry of full
  if (im.ximg.empty()) {
    CHECK(im.x_hot == 0 && im.x_rec == 0 && im.xr_off == 0 && im.ximg_bytes == 0, "%s: ximg scalars", what);
    return;
  }
  CHECK(!im.full_u32 && im.ximg_bytes == im.ximg.size() && im.ximg.size() <= kLongDfaLdsBytes &&
            im.x_hot + im.x_rec == S && im.xr_off % 8 == 0 &&
            size_t(im.xr_off) + 8 * size_t(im.x_rec) <= im.ximg.size(),
        "%s: ximg layout", what);
  const uint32_t rows = im.xr_off / (2 * K);
  auto hot = [&](uint32_t row, uint32_t k) {
    uint16_t x;
    memcpy(&x, im.ximg.data() + 2 * (size_t(row) * K + k), 2);
    return uint32_t(x);
  };
  for (uint32_t s = 0; s < S; ++s)
    for (uint32_t k = 0; k < K; ++k) {
      uint32_t t;
      if (s < im.x_hot) {
        t = hot(s, k);
      } else {
        DfaXRec r;
        memcpy(&r, im.ximg.data() + im.xr_off + 8 * size_t(s - im.x_hot), 8);
        CHECK((r.x & 0xffffu) < rows, "%s: default row of state %u", what, s);
        t = hot(r.x & 0xffffu, k);
        t = k == (r.x >> 24) ? (r.y >> 16) : t;
        t = k == ((r.x >> 16) & 0xffu) ? (r.y & 0xffffu) : t;
      }
      CHECK(t == full(s, k), "%s: ximg entry (%u, %u)", what, s, k);
    }
}

void check_common(const Blob& b, const PatternImage& im, const char* what) {
  const size_t ne = size_t(b.h.nstates) * b.h.nclasses;
  CHECK(im.table_bytes == im.table.size() && im.table.size() % 16 == 0 && !im.table.empty(), "%s: table size", what);
  CHECK(im.flags == b.h.flags && im.nstates == b.h.nstates, "%s: header", what);
  CHECK(im.h_trans.size() == ne && memcmp(im.h_trans.data(), b.trans(), 4 * ne) == 0 &&
            memcmp(im.h_cls, b.h.byte_class, 256) == 0 && im.h_nstates == b.h.nstates &&
            im.h_nclasses == b.h.nclasses && im.h_start == b.h.start && im.h_start_m == b.h.start_m,
        "%s: the carry walk's DFA", what);
  const bool longs = im.step_kind != kStepFilter && b.h.nstates <= 256;
  CHECK((im.long_states != 0) == longs && im.long_tbl.empty() == !longs && im.st2id.empty() == !longs,
        "%s: long-line table present", what);
  if (longs) {
    CHECK(im.long_states == b.h.nstates && im.long_start_m == b.h.start_m &&
              im.long_tbl.size() == size_t(b.h.nstates) * 256,
          "%s: long-line scalars", what);
    for (uint32_t s = 0; s < b.h.nstates; ++s)
      for (int c = 0; c < 256; ++c)
        CHECK(im.long_tbl[size_t(s) * 256 + c] == b.trans()[size_t(s) * b.h.nclasses + b.h.byte_class[c]],
              "%s: long_tbl (%u, %d)", what, s, c);
    for (uint32_t x : im.st2id) CHECK(x < b.h.nstates, "%s: st2id range", what);
  }
  const bool partial = (b.h.flags & DGREP_DFA_PARTIAL) != 0;
  CHECK(im.nfa.empty() == !partial && im.nfa.size() * 4 == b.h.nfa_bytes, "%s: nfa", what);
  if (partial)
    CHECK(memcmp(im.nfa.data(), b.trans() + ne, b.h.nfa_bytes) == 0 && im.nfa_words == im.nfa[2] &&
              im.step_kind == kStepFilter && im.full.empty(),
          "%s: nfa program", what);
  CHECK(im.full.empty() == !(im.step_kind == kStepFilter && !partial), "%s: full present", what);
  if (!im.full.empty()) check_full(b, im, what);
}

void check_walks(const Blob& b, const PatternImage& im, const std::vector<uint8_t>& corpus, const char* what) {
  const bool partial = (b.h.flags & DGREP_DFA_PARTIAL) != 0;
  for (int shift = 0; shift < 2; ++shift) {
    const std::vector<uint8_t> d(corpus.begin() + shift, corpus.end());
    std::vector<uint8_t> blob_cand, cand;
    const std::vector<uint32_t> want = walk_blob(b, d, partial ? b.h.nstates - 1 : UINT32_MAX, &blob_cand);
    std::vector<uint32_t> got;
    bool ok = false;
    switch (im.step_kind) {
      case kStepSheng8: ok = walk_sheng(b, im, d, &got); break;
      case kStepTable: ok = walk_table(b, im, d, &got); break;
      case kStepPair: ok = walk_pair(b, im, d, &got); break;
      case kStepFilter: ok = walk_filter(b, im, d, &got, &cand); break;
    }
    CHECK(ok, "%s: the image broke its stepper's walk (shift %d)", what, shift);
    if (!partial) {
      CHECK(got == want, "%s: %zu matching lines, the blob gives %zu (shift %d)", what, got.size(), want.size(), shift);
      continue;
    }
    // a partial blob: a line the filter decides is decided as the blob does, and
    // every line that reaches the blob's CAND is a candidate
    CHECK(cand.size() == blob_cand.size(), "%s: line count", what);
    size_t g = 0, w = 0;
    for (uint32_t line = 1; line <= cand.size(); ++line) {
      const bool gm = g < got.size() && got[g] == line, wm = w < want.size() && want[w] == line;
      g += gm;
      w += wm;
      CHECK(!blob_cand[line - 1] || cand[line - 1], "%s: line %u reaches CAND, the filter decided it", what, line);
      CHECK(cand[line - 1] || gm == wm, "%s: line %u decided against the blob", what, line);
    }
  }
}

void print_image(const std::string& tag, const PatternImage& im) {
  printf("%s kind=%d table=%zu start=%u start_m=%u nclasses=%u cand_end=%u pair=%u,%u,%u,%u nl=%u,%u empty=%d "
         "x_hot=%u x_rec=%u xr_off=%u blob=%u,%u,%u,%u u32=%d verify_hot=%u nfa_words=%u long=%u,%u seeds=",
         tag.c_str(), im.step_kind, im.table.size(), im.start, im.start_m, im.nclasses, im.cand_end, im.pair_args.t1,
         im.pair_args.thr, im.pair_args.div, im.pair_args.w32, im.sheng_nl_lo, im.sheng_nl_hi,
         int(im.empty_line_matches), im.x_hot, im.x_rec, im.xr_off, im.blob_start, im.blob_start_m, im.blob_matched,
         im.blob_dead, int(im.full_u32), im.verify_hot, im.nfa_words, im.long_states, im.long_start_m);
  for (size_t i = 0; i < im.long_seed.size(); ++i) printf("%s%u", i ? "," : "", im.long_seed[i]);
  printf(" crc table=%08x full=%08x ximg=%08x nfa=%08x long_tbl=%08x st2id=%08x h_trans=%08x cls=%08x\n",
         crc_of(im.table), crc_of(im.full), crc_of(im.ximg), crc_of(im.nfa), crc_of(im.long_tbl), crc_of(im.st2id),
         crc_of(im.h_trans), crc32(im.h_cls, 256));
}

// the refusal a (blob, force) pair must get, if its message names the reason at all
void check_refusal(const Pattern& p, const Blob& b, const Force& f, int rc, const std::string& err) {
  const bool partial = (b.h.flags & DGREP_DFA_PARTIAL) != 0;
  const std::string tag = p.name + " force " + std::to_string(f.force) + ":" + std::to_string(f.cap);
  const std::string needs =
      "dgrep_load_dfa: a DFA of " + std::to_string(b.h.nstates) + " states needs the filter stepper";
  CHECK(rc == DGREP_E_UNSUPPORTED, "%s: refused with %d", tag.c_str(), rc);
  if (partial && (f.force == 2 || f.force == 3)) CHECK(err == kMsgPartial, "%s: %s", tag.c_str(), err.c_str());
  else if (f.force == 3) CHECK(err == kMsgPair, "%s: %s", tag.c_str(), err.c_str());
  else if (f.force == 4 || partial) CHECK(err == kMsgFilter && f.cap == 3, "%s: %s", tag.c_str(), err.c_str());
  else CHECK(err == needs && b.h.nstates > 256 && (f.force == 2 || f.cap == 3), "%s: %s", tag.c_str(), err.c_str());
}

}  // namespace

int main(int argc, char** argv) {
  bool print = false, check = true, auto_only = false;
  const char* path = PATTERNS_FILE;
  for (int i = 1; i < argc; ++i) {
    if (!strcmp(argv[i], "print")) print = true, check = false;
    else if (!strcmp(argv[i], "print-auto")) print = auto_only = true, check = false;
    else if (!strcmp(argv[i], "check-print")) print = true;
    else path = argv[i];
  }
  const std::vector<Pattern> patterns = read_patterns(path);
  if (patterns.empty()) {
    fprintf(stderr, "%s: %zu patterns\n", path, patterns.size());
    return 2;
  }
  size_t built = 0, refused = 0, seen_pair_refusal = 0, seen_rows3 = 0, seen_partial = 0, seen_needs = 0;
  for (const Pattern& p : patterns) {
    Blob b;
    char cerr[256] = "";
    const int crc = p.budget ? dgrep_compile_budget(p.text.data(), p.text.size(), p.budget, &b.p, &b.n, cerr, sizeof cerr)
                             : dgrep_compile(p.text.data(), p.text.size(), &b.p, &b.n, cerr, sizeof cerr);
    if (crc != DGREP_OK) {
      fprintf(stderr, "%s: compile failed (%d): %s\n", p.name.c_str(), crc, cerr);
      return 2;
    }
    memcpy(&b.h, b.p, sizeof b.h);
    const bool partial = (b.h.flags & DGREP_DFA_PARTIAL) != 0;
    const std::vector<uint8_t> corpus = make_corpus(p.hit);
    if (check) {
      std::vector<uint8_t> blob_cand;
      const std::vector<uint32_t> want = walk_blob(b, corpus, partial ? b.h.nstates - 1 : UINT32_MAX, &blob_cand);
      size_t cands = 0;
      for (uint8_t x : blob_cand) cands += x;
      if (corpus.size() >= 16384 || (want.empty() && !cands)) {
        fprintf(stderr, "%s: a corpus of %zu bytes with %zu matching lines\n", p.name.c_str(), corpus.size(), want.size());
        return 2;
      }
    }
    for (const Force& f : kForces) {
      if (auto_only && (f.force || f.cap)) continue;
      PatternImage im;
      std::string err;
      const int rc = build_pattern_image(b.p, b.n, f.force, f.cap ? f.cap : UINT32_MAX, &im, &err);
      const std::string tag = p.name + " " + std::to_string(f.force) + ":" + std::to_string(f.cap);
      if (rc != DGREP_OK) {
        ++refused;
        if (print) printf("%s refused %d %s\n", tag.c_str(), rc, err.c_str());
        if (!check) continue;
        check_refusal(p, b, f, rc, err);
        seen_pair_refusal += p.name == "cell:table-auto-32" && f.force == 3;
        seen_rows3 += f.force == 4 && f.cap == 3;
        seen_partial += partial && (f.force == 2 || f.force == 3);
        seen_needs += p.name == "cell:filter-257" && f.force == 0 && f.cap == 3;
        continue;
      }
      ++built;
      if (print) print_image(tag, im);
      if (!check) continue;
      if (f.force == 0 && f.cap == 0) {
        // nothing forced: every blob loads, on the stepper its size asks for
        const int kind = im.step_kind;
        if (partial ? kind != kStepFilter
                    : (b.h.nstates <= DGREP_SHENG_MAX_STATES && kind != kStepSheng8) ||
                          (b.h.nstates > 256 && kind != kStepPair && kind != kStepFilter)) {
          fprintf(stderr, "FAIL %s: kind %d\n", tag.c_str(), kind);
          ++g_fail;
        }
      }
      if ((f.force == 2 && im.step_kind != kStepTable) || (f.force == 3 && im.step_kind != kStepPair) ||
          (f.force == 4 && im.step_kind != kStepFilter)) {
        fprintf(stderr, "FAIL %s: forced, kind %d\n", tag.c_str(), im.step_kind);
        ++g_fail;
      }
      check_common(b, im, tag.c_str());
      check_walks(b, im, corpus, tag.c_str());
    }
    if (check && p.name == "cell:pair-9") {
      // a blob with a transition out of range: refused whole, as a malformed blob
      std::vector<uint8_t> bad(static_cast<const uint8_t*>(b.p), static_cast<const uint8_t*>(b.p) + b.n);
      const uint32_t out_of_range = b.h.nstates;
      memcpy(bad.data() + sizeof b.h + 4 * (size_t(b.h.nclasses) + 1), &out_of_range, 4);
      void* heap = malloc(bad.size());
      memcpy(heap, bad.data(), bad.size());
      PatternImage im;
      std::string err;
      const int rc = build_pattern_image(heap, bad.size(), 0, UINT32_MAX, &im, &err);
      free(heap);
      if (rc != DGREP_E_INVALID || err != kMsgBlob) {
        fprintf(stderr, "FAIL transition out of range: %d %s\n", rc, err.c_str());
        ++g_fail;
      }
      // and a cut-off blob
      if (build_pattern_image(b.p, b.n - 1, 0, UINT32_MAX, &im, &err) != DGREP_E_INVALID || err != kMsgBlob) ++g_fail;
    }
    dgrep_blob_free(b.p);
  }
  if (!check) return 0;
  if (!seen_pair_refusal || seen_rows3 != patterns.size() || !seen_partial || !seen_needs) {
    fprintf(stderr, "FAIL: refusals seen: pair %zu, rows 3 %zu of %zu, partial %zu, needs-filter %zu\n",
            seen_pair_refusal, seen_rows3, patterns.size(), seen_partial, seen_needs);
    ++g_fail;
  }
  if (g_fail) {
    fprintf(stderr, "%d checks failed\n", g_fail);
    return 1;
  }
  printf("pattern_image OK %zu built, %zu refused\n", built, refused);
  return 0;
}
