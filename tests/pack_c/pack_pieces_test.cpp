// pack_pieces_test.cpp — the packing ingest's piece arithmetic (csrc/runtime/
// pack_pieces.h) under AddressSanitizer + UBSan, on the CPU, as a program of
// its own (not loaded into Python):
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I distributed-grep_amd/csrc/runtime tests/pack_c/pack_pieces_test.cpp -o pack_pieces_test
//   ./pack_pieces_test
//
// Every piece is assembled into a heap buffer of exactly the piece's length
// (so a segment one byte too long is a heap overflow the sanitizer reports),
// and the assembled pieces are compared with the plain concatenation
// s_0 '\n' s_1 '\n' ... s_{k-1}. Source splits are heap copies of their exact
// length for the same reason. The ingest's threaded host copy and the k = 1
// (single buffer) source are driven the same way, further down.
// Exit status 0 and "pack_pieces OK" = pass.
#include <stdio.h>
#include <stdlib.h>

#include <random>
#include <string>
#include <vector>

#include "pack_pieces.h"

using dgrep::PackCursor;
using dgrep::PackSeg;

static int failures = 0;

static void check(const std::vector<std::string>& splits, size_t piece, const char* what) {
  const size_t k = splits.size();
  std::vector<uint8_t*> data(k, nullptr);
  std::vector<size_t> n(k);
  std::string want;
  for (size_t i = 0; i < k; ++i) {
    n[i] = splits[i].size();
    if (n[i]) {  // an empty split may come with a null pointer
      data[i] = static_cast<uint8_t*>(malloc(n[i]));
      memcpy(data[i], splits[i].data(), n[i]);
    }
    want += splits[i];
    if (i + 1 < k) want += '\n';
  }
  size_t total = 0;
  if (!dgrep::pack_total(n.data(), k, &total) || total != want.size()) {
    fprintf(stderr, "%s piece %zu: pack_total %zu, want %zu\n", what, piece, total, want.size());
    ++failures;
  }
  std::string got;
  PackCursor cur;
  std::vector<PackSeg> segs;
  for (size_t off = 0; off < total; off += piece) {
    const size_t len = piece < total - off ? piece : total - off;
    uint8_t* dst = static_cast<uint8_t*>(malloc(len));
    memset(dst, 0xEE, len);
    dgrep::pack_piece_segments(n.data(), k, &cur, len, &segs);
    size_t covered = 0;
    for (const PackSeg& s : segs) {
      if (s.dst_off != covered || s.len == 0 || s.dst_off + s.len > len ||
          (s.split == dgrep::kPackSeparator ? s.len != 1 : s.src_off + s.len > n[s.split])) {
        fprintf(stderr, "%s piece %zu at %zu: bad segment\n", what, piece, off);
        ++failures;
      }
      covered += s.len;
      dgrep::pack_copy_segment(data.data(), s, dst);
    }
    if (covered != len) {
      fprintf(stderr, "%s piece %zu at %zu: segments cover %zu of %zu bytes\n", what, piece, off, covered, len);
      ++failures;
    }
    got.append(reinterpret_cast<char*>(dst), len);
    free(dst);
  }
  // nothing is left: one more request yields no segment
  dgrep::pack_piece_segments(n.data(), k, &cur, 16, &segs);
  if (!segs.empty() || got != want) {
    fprintf(stderr, "%s piece %zu: assembled bytes differ from the concatenation\n", what, piece);
    ++failures;
  }
  for (uint8_t* p : data) free(p);
}

// The threaded host copy (pack_copy_threaded / pack_copy_segment with T
// threads): `len` bytes from an exact-size heap source into an exact-size heap
// destination, compared with memcpy's result. A thread that wrote past len, or
// read past the source, is a heap overflow.
static void check_copy(size_t len, int T) {
  uint8_t* src = static_cast<uint8_t*>(malloc(len ? len : 1));
  uint8_t* dst = static_cast<uint8_t*>(malloc(len ? len : 1));
  uint8_t* want = static_cast<uint8_t*>(malloc(len ? len : 1));
  for (size_t i = 0; i < len; ++i) src[i] = uint8_t(i * 2654435761u >> 13);
  memset(dst, 0xEE, len ? len : 1);
  memset(want, 0xEE, len ? len : 1);
  if (len) memcpy(want, src, len);
  dgrep::pack_copy_threaded(dst, src, len, T);
  if (memcmp(dst, want, len ? len : 1) != 0) {
    fprintf(stderr, "pack_copy_threaded len %zu T %d: bytes differ from memcpy\n", len, T);
    ++failures;
  }
  // the same run as one segment of a piece, behind 3 bytes of it
  if (len) {
    uint8_t* piece = static_cast<uint8_t*>(malloc(len + 3));
    memset(piece, 0xEE, 3);
    const uint8_t* data[1] = {src};
    dgrep::pack_copy_segment(data, PackSeg{0, 0, 3, len}, piece, T);
    if (memcmp(piece + 3, want, len) != 0 || piece[0] != 0xEE || piece[2] != 0xEE) {
      fprintf(stderr, "pack_copy_segment len %zu T %d: bytes differ from memcpy\n", len, T);
      ++failures;
    }
    free(piece);
  }
  free(src);
  free(dst);
  free(want);
}

// A separator segment is one byte whatever T is: into a 1-byte heap piece.
static void check_separator(int T) {
  uint8_t* piece = static_cast<uint8_t*>(malloc(1));
  piece[0] = 0xEE;
  dgrep::pack_copy_segment(nullptr, PackSeg{dgrep::kPackSeparator, 0, 0, 1}, piece, T);
  if (piece[0] != '\n') {
    fprintf(stderr, "separator segment T %d: not a newline\n", T);
    ++failures;
  }
  free(piece);
}

// A single buffer is k = 1: taken piece by piece through pack_piece_segments it
// gives exactly one segment per non-empty piece, at piece offset 0, and the
// pieces reproduce the buffer (with or without the separator rule, which a
// single buffer never meets). This is what lets the one-buffer ingest be the
// packed one.
static void check_single(size_t n0, size_t piece, int T) {
  uint8_t* src = static_cast<uint8_t*>(malloc(n0 ? n0 : 1));
  for (size_t i = 0; i < n0; ++i) src[i] = uint8_t(i * 40503u >> 7);
  const uint8_t* data[1] = {src};
  const size_t n[1] = {n0};
  for (int sep = 0; sep < 2; ++sep) {
    std::string got;
    PackCursor cur;
    std::vector<PackSeg> segs;
    for (size_t off = 0; off < n0; off += piece) {
      const size_t len = piece < n0 - off ? piece : n0 - off;
      uint8_t* dst = static_cast<uint8_t*>(malloc(len));
      dgrep::pack_piece_segments(n, 1, &cur, len, &segs, sep != 0);
      if (segs.size() != 1 || segs[0].split != 0 || segs[0].src_off != off || segs[0].dst_off != 0 ||
          segs[0].len != len) {
        fprintf(stderr, "single buffer %zu piece %zu at %zu: not one whole segment\n", n0, piece, off);
        ++failures;
      }
      for (const PackSeg& s : segs) dgrep::pack_copy_segment(data, s, dst, T);
      got.append(reinterpret_cast<char*>(dst), len);
      free(dst);
    }
    dgrep::pack_piece_segments(n, 1, &cur, 16, &segs, sep != 0);
    if (!segs.empty() || got.size() != n0 || memcmp(got.data(), src, n0) != 0) {
      fprintf(stderr, "single buffer %zu piece %zu: the pieces do not reproduce it\n", n0, piece);
      ++failures;
    }
  }
  free(src);
}

int main() {
  const std::vector<std::string> fixed = {
      "", "\n", "error", "error\n", "", "", "", "x\nerror", "\nerror\n\n", "key\nk\n", "k", "\n\n", "",
      "abc \xe2\x82", "\xac def\n", "", "", "k\n", "\n", "", std::string(5000, 'a') + "error" + std::string(5000, 'b'), ""};
  std::vector<std::vector<std::string>> lists = {fixed, {""}, {"", ""}, {"k"}, {"", "k"}, {"k", ""}, {"\n"},
                                                 std::vector<std::string>(300, ""), std::vector<std::string>(300, "\n")};
  std::mt19937 rng(20240);
  const char* alpha[] = {"a", "e", "r", "\n", "\n", "\xe2\x82\xac", "\xff", "error", "key ", ""};
  for (int l = 0; l < 6; ++l) {
    std::vector<std::string> v(rng() % 400 + 1);
    for (std::string& s : v)
      for (unsigned j = rng() % 41; j > 0; --j) s += alpha[rng() % 10];
    if (l & 1) v.insert(v.begin() + v.size() / 2, std::string(20000, 'x'));  // a split over several 4096-byte pieces
    lists.push_back(v);
  }
  for (const auto& splits : lists)
    for (size_t piece : {size_t(1), size_t(7), size_t(4096)}) check(splits, piece, "list");
  // lengths whose sum overflows are refused
  const size_t big[2] = {~size_t(0) - 1, 5};
  size_t t = 0;
  if (dgrep::pack_total(big, 2, &t)) {
    fprintf(stderr, "pack_total accepted an overflowing sum\n");
    ++failures;
  }
  // the threaded copy: the single-copy lengths, the 4096-byte part edges, the 1 MiB threshold
  const size_t MiB = size_t(1) << 20;
  for (size_t len : {size_t(0), size_t(1), size_t(4095), size_t(4096), size_t(4097), MiB - 1, MiB, MiB + 1})
    for (int T : {1, 4}) check_copy(len, T);
  // more threads than 4096-byte parts (3 MiB + 5 has 769): no empty thread, nothing past len
  for (int T : {1, 2, 3, 7, 256}) check_copy(3 * MiB + 5, T);
  check_copy(5 * 4096 + 1 + MiB, 1 << 20);
  for (int T : {1, 4}) check_separator(T);
  for (size_t piece : {size_t(1), size_t(7), size_t(4096), size_t(100000)}) check_single(20011, piece, 4);
  check_single(2 * MiB + 3, MiB + 4097, 3);  // pieces above the threaded copy's threshold
  check_single(0, 4096, 4);
  if (failures) return 1;
  printf("pack_pieces OK (%zu split lists x 3 piece sizes)\n", lists.size());
  return 0;
}
