// pattern_image.h — everything a loaded pattern is, built on the host.
//
// build_pattern_image turns a compiled blob (dgrep_blob.h) into a PatternImage:
// the stepper it runs on and that stepper's LDS image, and what the passes
// after the scan read -- the whole DFA renumbered breadth-first with its
// absorbing states, lookback seeds and default-row image (filter stepper), the
// NFA program (partial blobs), the long-line table (<= 256 states) and the
// plain DFA of the carry walk. It decides which stepper a DFA gets; no other
// file does. dgrep_load_dfa uploads the buffers and commits the rest.
//
// Plain C++17 with no HIP call in it, so a stand-alone program drives it under
// a sanitizer (tests/pattern_image_c/pattern_image_test.cpp). The layout
// constants are in kernels/pattern_layout.h and, for the pair stepper,
// kernels/scan_common.h.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <utility>
#include <vector>

#include "../../../include/dgrep.h"
#include "../../../include/dgrep_blob.h"
#include "../kernels/scan_common.h"

namespace dgrep {

struct PatternImage {
  // the stepper and its image: what a scan launches with
  int step_kind = kStepTable;
  std::vector<uint8_t> table;  // the stepper's LDS image (see the builders below)
  uint32_t table_bytes = 0;    // its size (kept when the bytes are dropped after the upload)
  uint32_t flags = 0, nstates = 0, start = 0, start_m = 0;  // start / start_m as the stepper holds them
  uint32_t nclasses = 0;       // kStepPair, kStepFilter: the image's class count
  PairArgs pair_args;
  uint32_t cand_end = UINT32_MAX;             // kStepFilter: CAND_END, premultiplied (none: UINT32_MAX)
  uint32_t sheng_nl_lo = 0, sheng_nl_hi = 0;  // kStepSheng8: V['\n']
  bool empty_line_matches = false;

  // kStepFilter on a whole DFA: the DFA for verify_kernel and the long_dfa_* kernels
  std::vector<uint8_t> full;  // [nstates][nclasses], breadth-first ids: u16, or u32 above 65535 states
  bool full_u32 = false;
  uint32_t blob_start = 0, blob_start_m = 0;  // start / start_m in full's ids
  uint32_t blob_matched = UINT32_MAX;          // the absorbing accepting state in full's ids (none: UINT32_MAX)
  uint32_t blob_dead = UINT32_MAX;             // the absorbing rejecting state (none: UINT32_MAX)
  std::vector<uint32_t> long_seed;             // lookback start states of long_dfa_seg1_kernel (full's ids)
  uint32_t verify_hot = 0;                     // leading entries of full verify_kernel keeps in LDS
  std::vector<uint8_t> ximg;                   // the whole-DFA LDS image (build_ximg; u16 DFAs that fit)
  uint32_t ximg_bytes = 0, x_hot = 0, x_rec = 0, xr_off = 0;

  // DGREP_DFA_PARTIAL: the NFA program (verify_nfa_kernel) and its position-set words
  std::vector<uint32_t> nfa;
  uint32_t nfa_words = 0;

  // long lines on the Sheng / pair / table steppers (<= 256 states): the
  // blob's u8 [S][256] table and stepper state index -> blob state
  std::vector<uint8_t> long_tbl;
  std::vector<uint32_t> st2id;
  uint32_t long_states = 0, long_start_m = 0;

  // the blob's plain DFA, kept on the host for a bounded stream's carry walk (kernels/carry.h)
  std::vector<uint32_t> h_trans;
  uint8_t h_cls[256] = {};
  uint32_t h_nstates = 0, h_nclasses = 0, h_start = 0, h_start_m = 0;

  // frees the vectors the device holds a copy of (dgrep_load_dfa, after the upload)
  void drop_uploaded() {
    std::vector<uint8_t>().swap(table);
    std::vector<uint8_t>().swap(full);
    std::vector<uint8_t>().swap(ximg);
    std::vector<uint32_t>().swap(nfa);
    std::vector<uint8_t>().swap(long_tbl);
    std::vector<uint32_t>().swap(st2id);
  }
};

// the kind handed to the scan entry points: the stepper, with kKindW32 for the
// pair stepper's u32-entry image
inline int launch_kind(const PatternImage& p) {
  return p.step_kind | (p.step_kind == kStepPair && p.pair_args.w32 ? kKindW32 : 0);
}

// The LDS image through which long_dfa_seg1_kernel and verify_kernel read a
// whole u16 DFA F ([S][K], breadth-first ids) with no HBM access on the chain:
// rows [0, H) whole; then one DfaXRec (pattern_layout.h) for each state in
// [H, S) -- its default = the resident row differing from its own in the
// fewest classes (exhaustive, stopping at one difference; config 4: 30 ms),
// with the <= 2 differing classes as exceptions; a state no resident row
// comes within two classes of gets its own row after the first H (an EXTRA
// row, its record's default, no exceptions). Layout: rows (H + X) * K u16,
// records at *xr_off (8-aligned). H is the most rows that leave room for
// everything within `budget`; false if even 64 rows do not (the kernels then
// keep the first rows and read the rest from HBM).
inline bool build_ximg(const uint16_t* F, uint32_t S, uint32_t K, uint32_t budget, std::vector<uint8_t>* img,
                       uint32_t* hot, uint32_t* xr_off) {
  const uint64_t row = 2ull * K;
  if (K >= kXNone || row <= 8 || budget < 8ull * S + 64 * row + 8) return false;
  uint64_t H = std::min<uint64_t>(S, (budget - 8 - 8ull * S) / (row - 8));
  for (int attempt = 0; attempt < 8 && H >= 64; ++attempt) {
    const uint64_t R = S - H;
    std::vector<DfaXRec> rec(R);
    std::vector<uint32_t> extra;
    for (uint64_t j = 0; j < R; ++j) {
      const uint16_t* f = F + (H + j) * K;
      uint32_t best = 3, bd = 0;
      for (uint64_t d = 0; d < H && best > 1; ++d) {
        const uint16_t* g = F + d * K;
        uint32_t diff = 0;
        for (uint32_t k = 0; k < K && diff < best; ++k) diff += f[k] != g[k];
        if (diff < best) { best = diff; bd = uint32_t(d); }
      }
      if (best > 2) {
        rec[j] = DfaXRec{uint32_t(H + extra.size()) | (kXNone << 16) | (kXNone << 24), 0u};
        extra.push_back(uint32_t(H + j));
        continue;
      }
      uint32_t cl[2] = {kXNone, kXNone}, nx[2] = {0, 0}, e = 0;
      const uint16_t* g = F + uint64_t(bd) * K;
      for (uint32_t k = 0; k < K; ++k)
        if (f[k] != g[k]) { cl[e] = k; nx[e] = f[k]; ++e; }
      rec[j] = DfaXRec{bd | (cl[0] << 16) | (cl[1] << 24), nx[0] | (nx[1] << 16)};
    }
    const uint64_t off = ((H + extra.size()) * row + 7) & ~7ull, bytes = (off + 8 * R + 15) & ~15ull;
    if (bytes > budget || H + extra.size() > 0xffffu) {
      H -= std::min<uint64_t>(H, (bytes - budget) / (row - 8) + 1 + extra.size());
      continue;
    }
    img->assign(bytes, 0);
    memcpy(img->data(), F, H * row);
    for (size_t x = 0; x < extra.size(); ++x) memcpy(img->data() + (H + x) * row, F + uint64_t(extra[x]) * K, row);
    if (R) memcpy(img->data() + off, rec.data(), 8 * R);  // (R == 0: the whole DFA is resident)
    *hot = uint32_t(H);
    *xr_off = uint32_t(off);
    return true;
  }
  return false;
}

// The pair stepper's LDS image (StepPair, scan_dfa.hip) from the blob's DFA:
// C u8 [256] (byte -> esz class), T2 u32 (u16 if the image exceeds 16 KiB) [S'][K][K] at kPairT2 (two
// bytes per lookup), T1 u16 [S'][K] (single bytes); states premultiplied to
// their T2 row's LDS address (kPairT2 + id * 2K^2). S' = S + shadows: a pair whose FIRST byte is a '\n'
// entering start_m hides that event in the state between its bytes, so it
// leads to shadow(y) -- a copy of y = T[start_m][c2] -- instead of y. Ids:
// the states other than start_m, then the shadows of y != start_m, then
// start_m, then shadow(start_m): a pair-end id >= first shadow holds an
// event. Returns false if the DFA does not fit (T2 > kPairMaxT2 bytes).
inline bool build_pair_image(const dgrep_blob_header& h, const uint32_t* trans, std::vector<uint8_t>* img, uint32_t* start,
                      uint32_t* start_m, PairArgs* pa, std::vector<uint32_t>* orig_out) {
  const uint32_t S = h.nstates, K = h.nclasses, M = h.start_m;
  const uint32_t cn = h.byte_class[uint8_t('\n')];
  auto T = [&](uint32_t s, uint32_t c) { return trans[size_t(s) * K + c]; };
  // shadow targets, in class order
  std::vector<uint32_t> shadow_of(S, UINT32_MAX);  // original state -> shadow id
  std::vector<uint32_t> targets;
  bool any_flag = false;
  for (uint32_t s = 0; s < S; ++s) any_flag = any_flag || T(s, cn) == M;
  if (any_flag)
    for (uint32_t c = 0; c < K; ++c) {
      const uint32_t y = T(M, c);
      if (std::find(targets.begin(), targets.end(), y) == targets.end()) targets.push_back(y);
    }
  const uint32_t Sp = S + uint32_t(targets.size());
  // T2 entry: u32 when the image fits kPairW32MaxImage, else u16. Bytes per T2
  // row: esz K^2, padded to an ODD number of dwords so that the same column of
  // different rows falls in different LDS banks
  auto row_of = [&](uint64_t esz) { return ((esz * K * K + 3) & ~3ull) | 4ull; };
  auto end_of = [&](uint64_t r) {
    const uint64_t t1 = (kPairT2 + r * Sp + 15) & ~15ull;
    return std::make_pair(t1, (t1 + 2ull * Sp * K + 15) & ~15ull);
  };
  uint32_t esz = DGREP_PAIR_T2_U32 && end_of(row_of(4)).second <= kPairW32MaxImage ? 4u : 2u;
  const uint64_t row = row_of(esz);
  if (row * Sp > kPairMaxT2) return false;
  const uint64_t t1_off = end_of(row).first, end = end_of(row).second;
  if (end > kPairMaxImage) return false;
  std::vector<uint32_t> id(S), orig(Sp);
  uint32_t next = 0;
  for (uint32_t s = 0; s < S; ++s)
    if (s != M) { id[s] = next; orig[next++] = s; }
  const bool m_shadow = std::find(targets.begin(), targets.end(), M) != targets.end();
  for (uint32_t y : targets)
    if (y != M) { shadow_of[y] = next; orig[next++] = y; }
  id[M] = next;
  orig[next++] = M;
  if (m_shadow) { shadow_of[M] = next; orig[next++] = M; }
  // ids S-1 .. S'-1: the shadows of y != start_m, start_m, shadow(start_m)
  const uint32_t thr_id = S - 1;
  auto premul = [&](uint32_t i) { return uint16_t(kPairT2 + uint64_t(i) * row); };
  img->assign(end, 0);
  uint8_t* const t2 = img->data() + kPairT2;
  uint16_t* t1 = reinterpret_cast<uint16_t*>(img->data() + t1_off);
  for (uint32_t i = 0; i < Sp; ++i) {
    const uint32_t x = orig[i];
    for (uint32_t c1 = 0; c1 < K; ++c1) {
      const uint32_t a = T(x, c1);
      const bool flagged = c1 == cn && a == M;
      t1[size_t(i) * K + c1] = premul(id[a]);
      for (uint32_t c2 = 0; c2 < K; ++c2) {
        const uint32_t y = T(a, c2);
        const uint16_t v = premul(flagged ? shadow_of[y] : id[y]);
        uint8_t* const e = t2 + size_t(i) * row + esz * (size_t(c1) * K + c2);
        if (esz == 4) {
          const uint32_t v32 = v;
          memcpy(e, &v32, 4);
        } else {
          memcpy(e, &v, 2);
        }
      }
    }
  }
  // one u8 table C[b] = esz class(b) at LDS 0; esz (K - 1) < 256; and (for
  // the pair's first byte) CK[b] = esz K class(b), u16 at kPairCK
  if (esz * (K - 1u) > 255u) return false;
  for (int b = 0; b < 256; ++b) {
    img->data()[b] = uint8_t(esz * h.byte_class[b]);
    const uint16_t ck = uint16_t(esz * K * h.byte_class[b]);
    memcpy(img->data() + kPairCK + 2 * b, &ck, 2);
  }
  *start = premul(id[h.start]);
  *start_m = premul(id[M]);
  *orig_out = orig;  // pair state index -> blob state (a shadow -> the state it copies)
  pa->t1 = uint32_t(t1_off);
  pa->thr = premul(thr_id);
  pa->div = uint32_t(row);
  pa->w32 = esz == 4 ? 1u : 0u;
  return true;
}

// The filter stepper's LDS image (StepFilter, scan_dfa.hip): byte classes (kFilterClassBytes),
// then u16 rows of the DFA's first
// R - 2 states in breadth-first order from start (start_m at depth 0), as many
// rows as kFilterImageBytes holds, plus CAND (every transition out of them;
// '\n' -> CAND_END) and CAND_END (start's row). Ids: kept states other than
// start_m, CAND, start_m, CAND_END; entries premultiplied by K. Returns false
// if not even start, start_m and their successors fit.
// `excluded`: a partial blob's CAND state (never kept, so every transition
// into it is a filter CAND too).
inline bool build_filter_image(const dgrep_blob_header& h, const uint32_t* trans, uint32_t row_cap, std::vector<uint8_t>* img,
                        uint32_t* start, uint32_t* start_m, uint32_t* cand_end, uint32_t excluded = UINT32_MAX) {
  const uint32_t S = h.nstates, K = h.nclasses, M = h.start_m;
  const uint32_t cn = h.byte_class[uint8_t('\n')];
  // row pitch P >= K entries with P / 2 odd (DGREP_FILTER_PITCH): consecutive
  // rows start an odd number of dwords apart, so the rows a wave's lanes sit in
  // cover the 32 banks in turn (a CPU model of config 4's chain reads: 5.8 ->
  // 5.6 LDS cycles per read)
  const uint32_t P = DGREP_FILTER_PITCH ? ((K + 1) & ~1u) + (((K + 1) & 2u) ? 0u : 2u) : K;
  // rows that fit (row_cap: dgrep_set_stepper's test knob)
  const uint32_t R = std::min<uint32_t>((kFilterImageBytes - kFilterClassBytes) / (2 * P), row_cap);
  if (R < 4 || uint64_t(R) * P > 65535) return false;
  std::vector<uint32_t> order;
  std::vector<uint8_t> seen(S, 0);
  auto visit = [&](uint32_t x) {
    if (!seen[x] && x != excluded) { seen[x] = 1; order.push_back(x); }
  };
  visit(h.start);
  visit(M);
  for (size_t q = 0; q < order.size(); ++q)
    for (uint32_t k = 0; k < K; ++k) visit(trans[size_t(order[q]) * K + k]);
  const bool part = excluded != UINT32_MAX;
  const uint32_t keep = std::min<uint32_t>(uint32_t(order.size()), S <= R && !part ? S : R - 2);
  if (keep < 2) return false;
  std::vector<uint32_t> id(S, UINT32_MAX);
  uint32_t next = 0;
  for (uint32_t i = 0; i < keep; ++i)
    if (order[i] != M) id[order[i]] = next++;
  const bool exact = keep == S && !part;  // the whole DFA fits: no candidates
  const uint32_t CAND = exact ? UINT32_MAX : next++;
  id[M] = next++;
  const uint32_t CEND = exact ? UINT32_MAX : next++;
  const uint32_t Sf = next;
  auto to = [&](uint32_t x) { return uint16_t((id[x] == UINT32_MAX ? CAND : id[x]) * P); };
  img->assign((kFilterClassBytes + size_t(Sf) * P * 2 + 15) & ~size_t(15), 0);
  for (int b = 0; b < 256; ++b) img->data()[b] = h.byte_class[b];
  uint16_t* rows = reinterpret_cast<uint16_t*>(img->data() + kFilterClassBytes);
  for (uint32_t i = 0; i < keep; ++i) {
    const uint32_t x = order[i];
    for (uint32_t k = 0; k < K; ++k) rows[size_t(id[x]) * P + k] = to(trans[size_t(x) * K + k]);
  }
  if (!exact) {
    for (uint32_t k = 0; k < K; ++k) {
      rows[size_t(CAND) * P + k] = uint16_t((k == cn ? CEND : CAND) * P);
      rows[size_t(CEND) * P + k] = to(trans[size_t(h.start) * K + k]);
    }
  }
  *start = id[h.start] * P;
  *start_m = id[M] * P;
  *cand_end = exact ? UINT32_MAX : CEND * P;
  return true;
}

// StepSheng8: V[b] = 8 bytes, byte s = next state of s on input byte b
inline void sheng_image(const dgrep_blob_header& h, const uint32_t* trans, PatternImage* c) {
  c->step_kind = kStepSheng8;
  // renumber so start_m is the highest state (the kernel tests a word's four
  // states for start_m with one max), and carry the start state replicated
  // in all four bytes: v_perm keeps a replicated selector replicated, so
  // every state on the chain is a clean 0x01010101 multiple
  const uint32_t S = h.nstates, top = S - 1;
  std::vector<uint32_t> id(S);
  for (uint32_t x = 0; x < S; ++x) id[x] = x;
  std::swap(id[h.start_m], id[top]);
  std::vector<uint8_t>& t = c->table;
  t.assign(256 * 8, 0);
  for (int b = 0; b < 256; ++b)
    for (uint32_t s = 0; s < S; ++s)
      t[size_t(b) * 8 + id[s]] = uint8_t(id[trans[size_t(s) * h.nclasses + h.byte_class[b]]]);
  c->start = id[h.start] * 0x01010101u;
  // V['\n'] for the long-line kernel (a line the split's end closes)
  c->sheng_nl_lo = c->sheng_nl_hi = 0;
  for (int k = 0; k < 4; ++k) {
    c->sheng_nl_lo |= uint32_t(t[size_t('\n') * 8 + k]) << (8 * k);
    c->sheng_nl_hi |= uint32_t(t[size_t('\n') * 8 + 4 + k]) << (8 * k);
  }
  c->start_m = top;
  c->st2id.assign(S, 0);
  for (uint32_t x = 0; x < S; ++x) c->st2id[id[x]] = x;
}

// StepTable: row s (stride kTableRow = 260, bank-staggered) holds
// trans[s][class(b)] at byte b
inline void table_image(const dgrep_blob_header& h, const uint32_t* trans, PatternImage* c) {
  c->step_kind = kStepTable;
  c->st2id.resize(h.nstates);
  for (uint32_t x = 0; x < h.nstates; ++x) c->st2id[x] = x;
  const size_t row = kTableRow;
  std::vector<uint8_t>& t = c->table;
  t.assign((size_t(h.nstates) * row + 15) & ~size_t(15), 0);
  for (uint32_t s = 0; s < h.nstates; ++s)
    for (int b = 0; b < 256; ++b) t[size_t(s) * row + size_t(b)] = uint8_t(trans[size_t(s) * h.nclasses + h.byte_class[b]]);
  c->start = h.start;
  c->start_m = h.start_m;
}

// The whole DFA for verify_kernel, renumbered breadth-first from start
// (start, start_m, then BFS) so its hot rows lead; u16 entries while the
// ids fit, u32 above 65535 states (up to the compiler's budget); and its LDS
// image (build_ximg) where it fits. Returns blob state -> breadth-first id.
inline std::vector<uint32_t> full_dfa(const dgrep_blob_header& h, const uint32_t* trans, PatternImage* c) {
  const uint32_t S = h.nstates, K = h.nclasses;
  std::vector<uint32_t> order, bid(S, UINT32_MAX);
  order.reserve(S);
  auto visit = [&](uint32_t x) {
    if (bid[x] == UINT32_MAX) { bid[x] = uint32_t(order.size()); order.push_back(x); }
  };
  visit(h.start);
  visit(h.start_m);
  for (size_t q = 0; q < order.size(); ++q)
    for (uint32_t k = 0; k < K; ++k) visit(trans[size_t(order[q]) * K + k]);
  for (uint32_t x = 0; x < S; ++x) visit(x);
  const size_t ne = size_t(S) * K;
  c->full_u32 = S > 65535;
  const size_t esz = c->full_u32 ? 4 : 2;
  std::vector<uint8_t>& full = c->full;
  full.resize(ne * esz);
  for (uint32_t n = 0; n < S; ++n)
    for (uint32_t k = 0; k < K; ++k) {
      const uint32_t x = bid[trans[size_t(order[n]) * K + k]];
      if (c->full_u32) reinterpret_cast<uint32_t*>(full.data())[size_t(n) * K + k] = x;
      else reinterpret_cast<uint16_t*>(full.data())[size_t(n) * K + k] = uint16_t(x);
    }
  c->verify_hot = uint32_t(std::min<size_t>(ne, kVerifyHotBytes / esz)) / K * K;
  if (!c->full_u32 &&
      build_ximg(reinterpret_cast<const uint16_t*>(full.data()), S, K, kLongDfaLdsBytes, &c->ximg, &c->x_hot,
                 &c->xr_off)) {
    c->x_rec = S - c->x_hot;
    c->ximg_bytes = uint32_t(c->ximg.size());
  }
  c->blob_start = bid[h.start];
  c->blob_start_m = bid[h.start_m];
  return bid;
}

// the absorbing states: MATCHED (every byte but '\n' loops, '\n' ->
// start_m; verification stops there) and DEAD (the same with '\n' ->
// start: a line there never matches)
inline void absorbing_states(const dgrep_blob_header& h, const uint32_t* trans, const std::vector<uint32_t>& bid,
                             PatternImage* c) {
  const uint32_t S = h.nstates, K = h.nclasses;
  c->blob_matched = c->blob_dead = UINT32_MAX;
  const uint32_t cn = h.byte_class[uint8_t('\n')];
  for (uint32_t x = 0; x < S; ++x) {
    bool absorbing = true;
    for (uint32_t k = 0; k < K && absorbing; ++k)
      if (k != cn && trans[size_t(x) * K + k] != x) absorbing = false;
    if (!absorbing) continue;
    if (trans[size_t(x) * K + cn] == h.start_m && c->blob_matched == UINT32_MAX) c->blob_matched = bid[x];
    if (trans[size_t(x) * K + cn] == h.start && c->blob_dead == UINT32_MAX) c->blob_dead = bid[x];
  }
}

// long lines' lookback seeds: start, then states spread over the first
// breadth-first ids -- the rows the seg kernel holds in LDS, so a seed's
// first steps do not take the cold path -- never an absorbing one: a DFA
// keeping a finite memory of the whole line (a parity, a flag) has seeds
// in each memory class with high probability, so a segment's guesses cover
// its true entry state (long_c4p: 4.7 -> 485 GB/s)
inline void long_seeds(const dgrep_blob_header& h, PatternImage* c) {
  const uint32_t S = h.nstates, K = h.nclasses;
  const size_t esz = c->full_u32 ? 4 : 2;
  const uint32_t NS = uint32_t(kLongSeeds);
  const uint32_t H = std::min<uint32_t>(S, std::max<uint32_t>(
                                               64, c->x_hot ? c->x_hot : kLongDfaHotBytes / (esz * K)));
  c->long_seed.assign(NS, c->blob_start);
  for (uint32_t i = 1; i < NS && H > 2; ++i) {
    uint32_t x = uint32_t(uint64_t(i) * (H - 1) / NS);
    for (uint32_t t = 0; t < S && (x == c->blob_matched || x == c->blob_dead || x == c->blob_start); ++t)
      x = (x + 1) % S;
    c->long_seed[i] = x;
  }
}

// long lines on the Sheng / pair / table steppers: the blob's u8 [S][256]
// table for the long-line kernels, with the image's st2id (DFAs of at most
// 256 states; above, the pair stepper's lanes read a long line on)
inline void long_table(const dgrep_blob_header& h, const uint32_t* trans, PatternImage* c) {
  if (c->step_kind == kStepFilter || h.nstates > 256 || c->st2id.empty()) {
    c->st2id.clear();
    return;
  }
  std::vector<uint8_t>& lt = c->long_tbl;
  lt.resize(size_t(h.nstates) * 256);
  for (uint32_t s = 0; s < h.nstates; ++s)
    for (int b = 0; b < 256; ++b) lt[size_t(s) * 256 + b] = uint8_t(trans[size_t(s) * h.nclasses + h.byte_class[b]]);
  c->long_states = h.nstates;
  c->long_start_m = h.start_m;
}

// A blob and dgrep_set_stepper's two knobs (force: 0 auto, 2 u8 table, 3 pair,
// 4 filter; filter_rows_cap: the filter's LDS rows) to the pattern's image.
// Touches nothing but *out (left in an unspecified state on a refusal) and
// *err (the message of a refusal). DGREP_E_INVALID: a malformed blob;
// DGREP_E_UNSUPPORTED: the forced stepper cannot run this DFA.
// The choice, in this order: pair if wanted (auto above the Sheng limit, or
// forced) and fitting; filter above 256 states, for a partial blob, or forced;
// Sheng up to its limit unless the table is forced; else the table.
inline int build_pattern_image(const void* blob, size_t n, int force, uint32_t filter_rows_cap, PatternImage* out,
                               std::string* err) {
  PatternImage* const c = out;
  *c = PatternImage();
  dgrep_blob_info info;
  if (dgrep_blob_info_get(blob, n, &info) != DGREP_OK) {
    *err = "dgrep_load_dfa: malformed blob";
    return DGREP_E_INVALID;
  }
  dgrep_blob_header h;
  memcpy(&h, blob, sizeof h);
  const uint32_t* trans = reinterpret_cast<const uint32_t*>(static_cast<const uint8_t*>(blob) + sizeof h);
  for (size_t i = 0; i < size_t(h.nstates) * h.nclasses; ++i)
    if (trans[i] >= h.nstates) {
      *err = "dgrep_load_dfa: transition out of range";
      return DGREP_E_INVALID;
    }
  // a partial DFA (DGREP_DFA_PARTIAL) runs only as a filter: its last state is
  // CAND, and the NFA program after `trans` verifies the lines that reach it
  const bool partial = (h.flags & DGREP_DFA_PARTIAL) != 0;
  if (partial && force != 0 && force != 4) {
    *err = "dgrep_load_dfa: a partial DFA (over the compiler's state budget) runs on the filter stepper only";
    return DGREP_E_UNSUPPORTED;
  }
  const bool want_pair =
      !partial && ((force == 0 && h.nstates > DGREP_SHENG_MAX_STATES && DGREP_PAIR_ENABLE) || force == 3);
  const bool pair_ok =
      want_pair && build_pair_image(h, trans, &c->table, &c->start, &c->start_m, &c->pair_args, &c->st2id);
  if (force == 3 && !pair_ok) {
    *err = "dgrep_load_dfa: the pair stepper's two-byte table does not fit this DFA";
    return DGREP_E_UNSUPPORTED;
  }
  const bool filter_ok = !pair_ok && ((force == 0 && (h.nstates > 256 || partial)) || force == 4) &&
                         build_filter_image(h, trans, filter_rows_cap, &c->table, &c->start, &c->start_m, &c->cand_end,
                                            partial ? h.nstates - 1 : UINT32_MAX);
  if ((force == 4 || partial) && !filter_ok) {
    *err = "dgrep_load_dfa: the filter stepper cannot hold this DFA's first states";
    return DGREP_E_UNSUPPORTED;
  }
  if (pair_ok) {
    c->step_kind = kStepPair;
    c->nclasses = h.nclasses;
  } else if (filter_ok && partial) {
    c->step_kind = kStepFilter;
    c->nclasses = h.nclasses;
    const uint32_t* prog = trans + size_t(h.nstates) * h.nclasses;
    if (h.nfa_bytes < 32 || prog[0] != DGREP_NFA_MAGIC || prog[1] > DGREP_NFA_MAX_POS) {
      *err = "dgrep_load_dfa: malformed NFA program";
      return DGREP_E_INVALID;
    }
    c->nfa_words = prog[2];
    c->nfa.assign(prog, prog + h.nfa_bytes / 4);
  } else if (filter_ok) {
    c->step_kind = kStepFilter;
    c->nclasses = h.nclasses;
    absorbing_states(h, trans, full_dfa(h, trans, c), c);
    long_seeds(h, c);
  } else if (h.nstates > 256) {
    // the filter holds any DFA's first states (build_filter_image): only its
    // forced row cap (dgrep_set_stepper) can leave a large DFA here
    *err = "dgrep_load_dfa: a DFA of " + std::to_string(h.nstates) + " states needs the filter stepper";
    return DGREP_E_UNSUPPORTED;
  } else if (h.nstates <= DGREP_SHENG_MAX_STATES && force != 2) {
    sheng_image(h, trans, c);
  } else {
    table_image(h, trans, c);
  }
  c->table_bytes = uint32_t(c->table.size());
  c->flags = h.flags;
  c->nstates = h.nstates;
  long_table(h, trans, c);
  c->empty_line_matches = trans[size_t(h.start) * h.nclasses + h.byte_class[uint8_t('\n')]] == h.start_m;
  // the plain DFA for the carry walk
  c->h_trans.assign(trans, trans + size_t(h.nstates) * h.nclasses);
  memcpy(c->h_cls, h.byte_class, 256);
  c->h_nstates = h.nstates;
  c->h_nclasses = h.nclasses;
  c->h_start = h.start;
  c->h_start_m = h.start_m;
  return DGREP_OK;
}

}  // namespace dgrep
