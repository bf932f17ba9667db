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
// length for the same reason. Exit status 0 and "pack_pieces OK" = pass.
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
  if (failures) return 1;
  printf("pack_pieces OK (%zu split lists x 3 piece sizes)\n", lists.size());
  return 0;
}
