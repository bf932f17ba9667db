// pack_nosep_test.cpp — the separator-less mode of the packing ingest's piece
// arithmetic (csrc/runtime/pack_pieces.h, pack_piece_segments(..., sep =
// false): the batch reduce's inputs laid back to back) under AddressSanitizer +
// UBSan, on the CPU, as a program of its own (not loaded into Python). As
// tests/pack_c/pack_pieces_test.cpp: every piece is assembled into a heap
// buffer of exactly its length and the pieces are compared with the plain
// concatenation s_0 s_1 ... s_{k-1}; no segment may be a separator. Exit
// status 0 and "pack_nosep OK" = pass.
#include <stdio.h>
#include <stdlib.h>

#include <random>
#include <string>
#include <vector>

#include "pack_pieces.h"

using dgrep::PackCursor;
using dgrep::PackSeg;

static int failures = 0;

static void check(const std::vector<std::string>& inputs, size_t piece) {
  const size_t k = inputs.size();
  std::vector<uint8_t*> data(k, nullptr);
  std::vector<size_t> n(k);
  std::string want;
  for (size_t i = 0; i < k; ++i) {
    n[i] = inputs[i].size();
    if (n[i]) {  // an empty input may come with a null pointer
      data[i] = static_cast<uint8_t*>(malloc(n[i]));
      memcpy(data[i], inputs[i].data(), n[i]);
    }
    want += inputs[i];
  }
  const size_t total = want.size();
  std::string got;
  PackCursor cur;
  std::vector<PackSeg> segs;
  for (size_t off = 0; off < total; off += piece) {
    const size_t len = piece < total - off ? piece : total - off;
    uint8_t* dst = static_cast<uint8_t*>(malloc(len));
    memset(dst, 0xEE, len);
    dgrep::pack_piece_segments(n.data(), k, &cur, len, &segs, false);
    size_t covered = 0;
    for (const PackSeg& s : segs) {
      if (s.split == dgrep::kPackSeparator || s.dst_off != covered || s.len == 0 || s.dst_off + s.len > len ||
          s.src_off + s.len > n[s.split]) {
        fprintf(stderr, "piece %zu at %zu: bad segment\n", piece, off);
        ++failures;
        continue;
      }
      covered += s.len;
      dgrep::pack_copy_segment(data.data(), s, dst);
    }
    if (covered != len) {
      fprintf(stderr, "piece %zu at %zu: segments cover %zu of %zu bytes\n", piece, off, covered, len);
      ++failures;
    }
    got.append(reinterpret_cast<char*>(dst), len);
    free(dst);
  }
  // nothing is left: one more request yields no segment
  dgrep::pack_piece_segments(n.data(), k, &cur, 16, &segs, false);
  if (!segs.empty() || got != want) {
    fprintf(stderr, "piece %zu: assembled bytes differ from the concatenation\n", piece);
    ++failures;
  }
  for (uint8_t* p : data) free(p);
}

int main() {
  const std::string line = "{\"Key\":\"a (line number #1)\",\"Value\":\"error\"}\n";
  std::vector<std::vector<std::string>> lists = {
      {""}, {"", ""}, {line}, {"", line}, {line, ""}, {"", "", line, "", "", line + line, ""},
      std::vector<std::string>(300, ""), std::vector<std::string>(300, line)};
  std::mt19937 rng(20241);
  for (int l = 0; l < 6; ++l) {
    std::vector<std::string> v(rng() % 400 + 1);
    for (std::string& s : v)
      for (unsigned j = rng() % 5; j > 0; --j) s += line.substr(rng() % 7);
    if (l & 1) v.insert(v.begin() + v.size() / 2, std::string(20000, 'x') + "\n");  // an input over several pieces
    lists.push_back(v);
  }
  for (const auto& inputs : lists)
    for (size_t piece : {size_t(1), size_t(7), size_t(4096)}) check(inputs, piece);
  if (failures) return 1;
  printf("pack_nosep OK (%zu input lists x 3 piece sizes)\n", lists.size());
  return 0;
}
