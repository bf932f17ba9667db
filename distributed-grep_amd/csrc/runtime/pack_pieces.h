// pack_pieces.h — piece arithmetic of the packing ingest (dgrep_scan_batch).
//
// The packed buffer P = s_0 '\n' s_1 '\n' ... '\n' s_{k-1} is never built on
// the host as a whole: the ingest fills one staging piece of P at a time from
// the runs of source splits and separator bytes that fall into it. This header
// makes no HIP call, so a stand-alone program can drive it under a sanitizer
// (tests/pack_c/pack_pieces_test.cpp).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <thread>
#include <vector>

namespace dgrep {

constexpr size_t kPackSeparator = ~size_t(0);

// `len` bytes of a piece at piece offset `dst_off`: bytes [src_off, src_off +
// len) of split `split`, or (split == kPackSeparator, len == 1) one '\n'.
struct PackSeg {
  size_t split;
  size_t src_off;
  size_t dst_off;
  size_t len;
};

// Where the next byte of P comes from: byte `off` of split `split`, with off ==
// n[split] standing for the separator after it (only when split < k - 1).
struct PackCursor {
  size_t split = 0;
  size_t off = 0;
};

// bytes of P, or false if the sum overflows size_t
inline bool pack_total(const size_t* n, size_t k, size_t* total) {
  size_t t = k ? k - 1 : 0;
  for (size_t i = 0; i < k; ++i) {
    if (n[i] > ~size_t(0) - t) return false;
    t += n[i];
  }
  *total = t;
  return true;
}

// The segments of the next `len` bytes of P from *cur on (the caller keeps len
// within what is left of P), in order; *cur moves past them. `sep` = false:
// the splits back to back with no separator byte (P is then their plain
// concatenation).
inline void pack_piece_segments(const size_t* n, size_t k, PackCursor* cur, size_t len, std::vector<PackSeg>* segs,
                                bool sep = true) {
  segs->clear();
  size_t done = 0;
  while (done < len && cur->split < k) {
    const size_t left = n[cur->split] - cur->off;
    if (left) {
      const size_t m = left < len - done ? left : len - done;
      segs->push_back(PackSeg{cur->split, cur->off, done, m});
      cur->off += m;
      done += m;
    } else {
      if (sep && cur->split + 1 < k) {
        segs->push_back(PackSeg{kPackSeparator, 0, done, 1});
        ++done;
      }
      ++cur->split;
      cur->off = 0;
    }
  }
}

// The host copy of the ingest: `len` bytes by at most T threads, each a
// 4096-aligned part; one memcpy when T == 1 or below 1 MiB.
inline void pack_copy_threaded(uint8_t* dst, const uint8_t* src, size_t len, int T) {
  if (T <= 1 || len < (size_t(1) << 20)) {
    if (len) memcpy(dst, src, len);
    return;
  }
  std::vector<std::thread> th;
  const size_t part = ((len + size_t(T) - 1) / size_t(T) + 4095) & ~size_t(4095);
  for (size_t a = 0; a < len; a += part) {
    const size_t m = part < len - a ? part : len - a;
    th.emplace_back([=] { memcpy(dst + a, src + a, m); });
  }
  for (auto& x : th) x.join();
}

// one segment into the piece at dst: a separator is one byte, a split's run is copied by T threads
inline void pack_copy_segment(const uint8_t* const* data, const PackSeg& s, uint8_t* dst, int T = 1) {
  if (s.split == kPackSeparator) dst[s.dst_off] = uint8_t('\n');
  else pack_copy_threaded(dst + s.dst_off, data[s.split] + s.src_off, s.len, T);
}

}  // namespace dgrep
