// escape_width_test.cpp — the local width rule (csrc/kernels/escape_width.h)
// against the sequential escaper it restates (encode_common.h, json_body), on
// the host under ASan + UBSan. For every input: the widths sum to
// json_body<false>, and writing every byte's expansion at the prefix offset of
// the widths gives json_body<true>'s bytes. Inputs: all strings of 1 and 2
// bytes; all strings of 3 and 4 bytes over the edge alphabet; 2,000 seeded
// random strings up to 64 bytes. Every input sits in a heap block of its exact
// size, so a read outside [0, L) is an ASan report.
//
// `escape_width_test --stream` checks nothing itself: it reads values from
// stdin, each a little-endian u32 length and that many bytes, and writes for
// each one a u32 length and json_body<true>'s bytes, then a u32 length and the
// bytes of escape_width_at + escape_put. tests/test_writer_edge_cases.py
// compares both with the oracle. The values sit in exact-size heap blocks too.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "encode_common.h"
#include "escape_width.h"

using dgrep::json_body;

static const uint8_t kEdge[] = {0x00, 0x22, 0x41, 0x7F, 0x80, 0x8F, 0x90, 0x9F, 0xA0, 0xA8, 0xA9, 0xBF,
                                0xC0, 0xC2, 0xDF, 0xE0, 0xE2, 0xED, 0xEF, 0xF0, 0xF4, 0xF5, 0xFF};
static const int kNEdge = int(sizeof kEdge);

static long g_checked = 0;

static bool check(const uint8_t* src, size_t L) {
  uint8_t* s = static_cast<uint8_t*>(malloc(L ? L : 1));  // exact size: ASan guards both ends
  memcpy(s, src, L);
  const uint64_t want_n = json_body<false>(s, L, nullptr);
  std::vector<uint8_t> want(want_n + 1), got(want_n + 1, 0xEE);
  json_body<true>(s, L, want.data());
  uint64_t o = 0;
  bool ok = true;
  for (size_t i = 0; i < L; ++i) {
    uint8_t w[7];
    const uint32_t width = dgrep::escape_width_at(s, L, i, w);
    const uint32_t after = uint32_t(L - 1 - i < 3 ? L - 1 - i : 3);
    if (o + width > want_n) { ok = false; break; }
    dgrep::escape_put(w, after, width, got.data() + o);
    o += width;
  }
  if (ok && o != want_n) ok = false;
  if (ok && memcmp(got.data(), want.data(), want_n) != 0) ok = false;
  if (!ok) {
    fprintf(stderr, "MISMATCH on");
    for (size_t i = 0; i < L; ++i) fprintf(stderr, " %02x", s[i]);
    fprintf(stderr, " (sum %llu, json_body %llu)\n", (unsigned long long)o, (unsigned long long)want_n);
  }
  free(s);
  ++g_checked;
  return ok;
}

static bool read_exact(void* p, size_t n) { return n == 0 || fread(p, 1, n, stdin) == n; }

static void write_block(const std::vector<uint8_t>& v, size_t n) {
  const uint32_t len = uint32_t(n);
  fwrite(&len, 4, 1, stdout);
  if (n) fwrite(v.data(), 1, n, stdout);
}

static int stream() {
  uint32_t len;
  long count = 0;
  while (fread(&len, 4, 1, stdin) == 1) {
    const size_t L = len;
    uint8_t* s = static_cast<uint8_t*>(malloc(L ? L : 1));
    if (!read_exact(s, L)) {
      fprintf(stderr, "value %ld is cut off\n", count);
      free(s);
      return 2;
    }
    const uint64_t n = json_body<false>(s, L, nullptr);
    std::vector<uint8_t> seq(n + 1), local(6 * L + 1, 0xEE);
    json_body<true>(s, L, seq.data());
    write_block(seq, n);
    uint64_t o = 0;
    for (size_t i = 0; i < L; ++i) {
      uint8_t w[7];
      const uint32_t width = dgrep::escape_width_at(s, L, i, w);
      const uint32_t after = uint32_t(L - 1 - i < 3 ? L - 1 - i : 3);
      dgrep::escape_put(w, after, width, local.data() + o);  // width <= 6: inside 6 * L
      o += width;
    }
    write_block(local, o);
    free(s);
    ++count;
  }
  fflush(stdout);
  fprintf(stderr, "streamed %ld values\n", count);
  return 0;
}

int main(int argc, char** argv) {
  if (argc > 1 && strcmp(argv[1], "--stream") == 0) return stream();
  bool ok = true;
  uint8_t b[64];
  for (int a = 0; a < 256; ++a) {
    b[0] = uint8_t(a);
    ok &= check(b, 1);
    for (int c = 0; c < 256; ++c) {
      b[1] = uint8_t(c);
      ok &= check(b, 2);
    }
  }
  for (int i0 = 0; i0 < kNEdge; ++i0)
    for (int i1 = 0; i1 < kNEdge; ++i1)
      for (int i2 = 0; i2 < kNEdge; ++i2) {
        b[0] = kEdge[i0]; b[1] = kEdge[i1]; b[2] = kEdge[i2];
        ok &= check(b, 3);
        for (int i3 = 0; i3 < kNEdge; ++i3) {
          b[3] = kEdge[i3];
          ok &= check(b, 4);
        }
      }
  uint64_t x = 0x9E3779B97F4A7C15ull;  // splitmix-style, seeded
  auto rnd = [&]() {
    x += 0x9E3779B97F4A7C15ull;
    uint64_t z = x;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
  };
  for (int t = 0; t < 2000; ++t) {
    const size_t L = size_t(rnd() % 65);
    for (size_t i = 0; i < L; ++i) {
      const uint64_t r = rnd();
      // half the bytes from the edge alphabet, so that sequences form and break
      b[i] = (r & 1) ? kEdge[(r >> 8) % kNEdge] : uint8_t(r >> 16);
    }
    ok &= check(b, L);
  }
  ok &= check(b, 0);
  printf("%s %ld inputs\n", ok ? "OK" : "FAILED", g_checked);
  return ok ? 0 : 1;
}
