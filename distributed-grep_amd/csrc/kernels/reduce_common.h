// reduce_common.h — what the single reduce (reduce.hip) and the batch reduce
// (reduce_batch.hip) share: the accepted line language (JSON string decoding,
// parse_line, KeyBytes), the two-pass SWAR newline positions, the block scan
// and the writer's dword builder. Everything sits in an unnamed namespace:
// each of the two files gets its own copy of the kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

namespace dgrep {
namespace {
constexpr int kRT = 256;

__device__ inline int hexval(uint32_t c) {
  if (c >= '0' && c <= '9') return int(c - '0');
  if (c >= 'a' && c <= 'f') return int(c - 'a' + 10);
  if (c >= 'A' && c <= 'F') return int(c - 'A' + 10);
  return -1;
}

// utf8.EncodeRune of r, packed low byte first; *nb: its length
__device__ __forceinline__ uint32_t pack_rune(uint32_t r, uint32_t* nb) {
  if (r < 0x80) { *nb = 1; return r; }
  if (r < 0x800) { *nb = 2; return (0xC0 | (r >> 6)) | ((0x80 | (r & 0x3F)) << 8); }
  if (r < 0x10000) {
    *nb = 3;
    return (0xE0 | (r >> 12)) | ((0x80 | ((r >> 6) & 0x3F)) << 8) | ((0x80 | (r & 0x3F)) << 16);
  }
  *nb = 4;
  return (0xF0 | (r >> 18)) | ((0x80 | ((r >> 12) & 0x3F)) << 8) | ((0x80 | ((r >> 6) & 0x3F)) << 16) |
         ((0x80 | (r & 0x3F)) << 24);
}

__device__ inline bool hex4(const uint8_t* s, uint64_t p, uint64_t end, uint32_t* r) {
  if (p + 4 > end) return false;
  uint32_t v = 0;
  for (int k = 0; k < 4; ++k) {
    const int d = hexval(s[p + k]);
    if (d < 0) return false;
    v = (v << 4) | uint32_t(d);
  }
  *r = v;
  return true;
}

// One unit of a JSON string body at s[i], i < end (the caller has dealt with
// '"' and bytes < 0x20): a plain byte, an escape, or a raw rune. Returns the
// index after it (UINT64_MAX if malformed); *w: the decoded UTF-8 bytes packed
// low byte first, *nb: how many. As encoding/json (decode.go unquoteBytes):
// a \u high surrogate followed by a \u low surrogate pairs up, any other
// surrogate escape is U+FFFD and consumes nothing after itself; a raw byte
// >= 0x80 goes through utf8.DecodeRune, so every byte of an invalid or
// truncated sequence is U+FFFD on its own (1 byte in, 3 bytes out). A
// continuation byte is 0x80..0xBF, so a sequence never reaches over the
// closing quote; `end` (the line's '\n') bounds the reads.
__device__ inline uint64_t json_unit(const uint8_t* s, uint64_t i, uint64_t end, uint32_t* w, uint32_t* nb) {
  const uint32_t b = s[i];
  if (b == '\\') {
    if (i + 1 >= end) return UINT64_MAX;
    const uint32_t e = s[i + 1];
    i += 2;
    *nb = 1;
    switch (e) {
      case '"': case '\\': case '/': *w = e; return i;
      case 'b': *w = 8; return i;
      case 'f': *w = 12; return i;
      case 'n': *w = 10; return i;
      case 'r': *w = 13; return i;
      case 't': *w = 9; return i;
      case 'u': break;
      default: return UINT64_MAX;
    }
    uint32_t r;
    if (!hex4(s, i, end, &r)) return UINT64_MAX;
    i += 4;
    if (r >= 0xD800 && r < 0xDC00) {
      uint32_t r2;
      if (i + 1 < end && s[i] == '\\' && s[i + 1] == 'u' && hex4(s, i + 2, end, &r2) && r2 >= 0xDC00 && r2 < 0xE000) {
        i += 6;
        r = 0x10000 + ((r - 0xD800) << 10) + (r2 - 0xDC00);
      } else {
        r = 0xFFFD;
      }
    } else if (r >= 0xDC00 && r < 0xE000) {
      r = 0xFFFD;
    }
    *w = pack_rune(r, nb);
    return i;
  }
  if (b < 0x80) {
    *w = b;
    *nb = 1;
    return i + 1;
  }
  // utf8.DecodeRune: first byte -> length and the second byte's range
  uint32_t need = 0, lo = 0x80, hi = 0xBF;
  if (b >= 0xC2 && b <= 0xDF) need = 2;
  else if (b >= 0xE0 && b <= 0xEF) { need = 3; if (b == 0xE0) lo = 0xA0; if (b == 0xED) hi = 0x9F; }
  else if (b >= 0xF0 && b <= 0xF4) { need = 4; if (b == 0xF0) lo = 0x90; if (b == 0xF4) hi = 0x8F; }
  bool ok = need != 0 && i + need <= end;
  uint32_t v = b;
  if (ok) {
    const uint32_t c = s[i + 1];
    ok = c >= lo && c <= hi;
    v |= c << 8;
  }
  for (uint32_t k = 2; ok && k < need; ++k) {
    const uint32_t c = s[i + k];
    ok = c >= 0x80 && c <= 0xBF;
    v |= c << (8 * k);
  }
  if (!ok) {
    *w = 0xBDBFEFu;  // U+FFFD
    *nb = 3;
    return i + 1;
  }
  *w = v;
  *nb = need;
  return i + need;
}

// Decodes the JSON string starting after its opening quote at s[i]; returns
// the index after the closing quote (or UINT64_MAX if malformed). WRITE:
// raw bytes go to out. *olen: raw length; *h: FNV-1a 64 of the raw bytes.
// *plain is cleared if the raw bytes are not the input bytes themselves (an
// escape, or a byte coerced to U+FFFD); it is never set.
template <bool WRITE>
__device__ uint64_t json_string(const uint8_t* s, uint64_t i, uint64_t end, uint8_t* out, uint64_t* olen,
                                uint64_t* h, bool* plain) {
  uint64_t o = 0, hh = 1469598103934665603ull;
  auto put = [&](uint32_t b) {
    if (WRITE) out[o] = uint8_t(b);
    ++o;
    hh = (hh ^ b) * 1099511628211ull;
  };
  while (i < end) {
    const uint32_t b = s[i];
    if (b == '"') {
      *olen = o;
      *h = hh;
      return i + 1;
    }
    if (b < 0x20) return UINT64_MAX;
    if (b != '\\' && b < 0x80) {
      put(b);
      ++i;
      continue;
    }
    uint32_t w, nb;
    const uint64_t ni = json_unit(s, i, end, &w, &nb);
    if (ni == UINT64_MAX) return UINT64_MAX;
    if (ni - i != nb) *plain = false;  // an escape is longer than its bytes, a coerced byte shorter
    for (uint32_t k = 0; k < nb; ++k) put((w >> (8 * k)) & 0xFFu);
    i = ni;
  }
  return UINT64_MAX;
}

__device__ inline bool lit(const uint8_t* s, uint64_t i, uint64_t end, const char* t) {
  for (; *t; ++t, ++i)
    if (i >= end || s[i] != uint8_t(*t)) return false;
  return true;
}

// Parses line [a, e) (e = its '\n'). Fills key/value raw extents in the
// decoded sense: returns false if malformed. *plain: both strings' raw bytes
// are their input bytes (the line is its frame around two byte ranges).
template <bool WRITE>
__device__ bool parse_line(const uint8_t* s, uint64_t a, uint64_t e, uint8_t* out, uint64_t* klen, uint64_t* vlen,
                           uint64_t* kh, bool* plain) {
  *plain = true;
  if (!lit(s, a, e, "{\"Key\":\"")) return false;
  uint64_t vh;
  uint64_t i = json_string<WRITE>(s, a + 8, e, out, klen, kh, plain);
  if (i == UINT64_MAX || !lit(s, i, e, ",\"Value\":\"")) return false;
  if (WRITE) out[*klen] = ' ';
  i = json_string<WRITE>(s, i + 10, e, WRITE ? out + *klen + 1 : nullptr, vlen, &vh, plain);
  if (i == UINT64_MAX || !lit(s, i, e, "}") || i + 1 != e) return false;
  if (WRITE) out[*klen + 1 + *vlen] = '\n';
  return true;
}

// The decoded bytes of a (valid) key, one at a time.
struct KeyBytes {
  const uint8_t* s;
  uint64_t i, end;
  uint32_t w = 0, nb = 0;
  __device__ KeyBytes(const uint8_t* s_, uint64_t i_, uint64_t end_) : s(s_), i(i_), end(end_) {}
  __device__ uint32_t next() {
    if (nb == 0) i = json_unit(s, i, end, &w, &nb);
    const uint32_t b = w & 0xFFu;
    w >>= 8;
    --nb;
    return b;
  }
};

// ---- newline positions: two coalesced passes over the input ------------
// (replaces a generic select over every byte). Block b owns bytes
// [b * kSeg, (b + 1) * kSeg); pass 1 counts its '\n' (16 B per thread and
// round, SWAR), an exclusive scan of the block counts gives each block's first
// index, pass 2 writes the positions in order (block-wide scan per round).
constexpr uint64_t kSeg = 256u << 10;

__device__ __forceinline__ uint32_t nl_bits4(uint32_t w) {  // bit k: byte k of w is '\n'
  const uint32_t x = w ^ 0x0a0a0a0au;
  const uint32_t m = ~(((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x) & 0x80808080u;
  return ((m >> 7) & 1u) | ((m >> 14) & 2u) | ((m >> 21) & 4u) | ((m >> 28) & 8u);
}
// bit k: byte q + k is a '\n' inside [lo, hi) (q 16-B aligned)
__device__ __forceinline__ uint32_t nl_piece(const uint8_t* s, uint64_t n, uint64_t q, uint64_t hi) {
  if (q >= hi) return 0;
  uint32_t m = 0;
  if (q + 16 <= n) {
    const uint4 v = *reinterpret_cast<const uint4*>(s + q);
    m = nl_bits4(v.x) | (nl_bits4(v.y) << 4) | (nl_bits4(v.z) << 8) | (nl_bits4(v.w) << 12);
  } else {
    for (uint32_t k = 0; q + k < n; ++k) m |= uint32_t(s[q + k] == '\n') << k;
  }
  if (q + 16 > hi) m &= (1u << uint32_t(hi - q)) - 1u;
  return m;
}

// block-wide exclusive scan of v (kRT threads); *total = the block's sum
__device__ __forceinline__ uint32_t block_excl_scan(uint32_t v, uint32_t* total) {
  __shared__ uint32_t wsum[kRT / 64];
  const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
  uint32_t x = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t t = __shfl_up(x, d, 64);
    if (lane >= uint32_t(d)) x += t;
  }
  if (lane == 63) wsum[w] = x;
  __syncthreads();
  uint32_t before = 0, all = 0;
#pragma unroll
  for (int k = 0; k < kRT / 64; ++k) {
    before += uint32_t(k) < w ? wsum[k] : 0u;
    all += wsum[k];
  }
  __syncthreads();
  *total = all;
  return before + x - v;
}

__global__ __launch_bounds__(kRT) void nl_count_kernel(const uint8_t* s, uint64_t n, uint64_t* counts) {
  const uint64_t lo = uint64_t(blockIdx.x) * kSeg, hi = min(n, lo + kSeg);
  uint32_t c = 0;
  for (uint64_t q = lo + 16u * threadIdx.x; q < hi; q += 16u * kRT) c += uint32_t(__popc(nl_piece(s, n, q, hi)));
  uint32_t total;
  (void)block_excl_scan(c, &total);
  if (threadIdx.x == 0) counts[blockIdx.x] = total;
}

__global__ __launch_bounds__(kRT) void nl_write_kernel(const uint8_t* s, uint64_t n, const uint64_t* offs,
                                                       uint64_t* nl) {
  const uint64_t lo = uint64_t(blockIdx.x) * kSeg, hi = min(n, lo + kSeg);
  uint64_t base = offs[blockIdx.x];
  for (uint64_t q0 = lo; q0 < hi; q0 += 16u * kRT) {
    const uint64_t q = q0 + 16u * threadIdx.x;
    uint32_t m = nl_piece(s, n, q, hi), total;
    const uint32_t ex = block_excl_scan(uint32_t(__popc(m)), &total);
    for (uint32_t k = 0; m; ++k) {
      const uint32_t b = uint32_t(__builtin_ctz(m));
      m &= m - 1u;
      nl[base + ex + k] = q + b;
    }
    base += total;
  }
}

__global__ void nl_total_kernel(const uint64_t* offs, const uint64_t* counts, uint64_t nblk, uint64_t* total) {
  *total = offs[nblk - 1] + counts[nblk - 1];
}

// ---- the writer's dword builder -------------------------------------------
// Lane `lane` of a wave builds output dwords (P >> 2) + lane + 64k of the
// plain line `key value\n` placed at out[P : P + ol): its raw key is
// s[a + 8 : a + 8 + kl) and its raw value s[a + 19 + kl : a + 19 + kl + vl). A
// dword wholly inside one range is one unaligned read (two aligned dwords +
// v_alignbyte), taken only while the second dword ends before n; a dword on a
// line edge holds only this line's bytes and is stored bytewise.
__device__ __forceinline__ void write_plain_dwords(const uint8_t* s, uint64_t n, uint8_t* out, uint32_t lane,
                                                   uint64_t Pr, uint64_t olr, uint64_t ar, uint64_t klr,
                                                   uint64_t vlr) {
  const uint64_t ks = ar + 8u, vs = ar + 19u + klr;  // raw key / value starts in the input
  for (uint64_t d = (Pr >> 2) + lane; d < ((Pr + olr + 3) >> 2); d += 64) {
    const uint64_t q0 = 4u * d;
    const int64_t o0 = int64_t(q0) - int64_t(Pr);
    uint64_t src = UINT64_MAX;
    if (o0 >= 0 && uint64_t(o0) + 4u <= klr) src = ks + uint64_t(o0);
    else if (o0 >= int64_t(klr) + 1 && uint64_t(o0) + 4u <= klr + 1u + vlr) src = vs + uint64_t(o0) - klr - 1u;
    if (src != UINT64_MAX && ((src + 3) | 3u) < n) {
      const uint32_t sh = uint32_t(src & 3u);
      const uint32_t* w = reinterpret_cast<const uint32_t*>(s + (src & ~uint64_t(3)));
      const uint32_t lo = w[0], hi = sh ? w[1] : 0u;
      *reinterpret_cast<uint32_t*>(out + q0) = __builtin_amdgcn_alignbyte(hi, lo, sh);
      continue;
    }
    uint32_t word = 0, have = 0;
#pragma unroll
    for (uint32_t b = 0; b < 4; ++b) {
      const int64_t ob = o0 + int64_t(b);
      if (ob < 0 || uint64_t(ob) >= olr) continue;
      const uint64_t o = uint64_t(ob);
      const uint32_t ch = o < klr ? s[ks + o] : o == klr ? uint32_t(' ') : o < klr + 1u + vlr ? s[vs + o - klr - 1u] : uint32_t('\n');
      word |= ch << (8 * b);
      have |= 1u << b;
    }
    if (have == 15u) {
      *reinterpret_cast<uint32_t*>(out + q0) = word;
    } else {
      for (uint32_t b = 0; b < 4; ++b)
        if (have & (1u << b)) out[q0 + b] = uint8_t(word >> (8 * b));
    }
  }
}

inline size_t a256(size_t x) { return (x + 255) & ~size_t(255); }
inline int grid_of(uint64_t n) { return int(std::min<uint64_t>((n + kRT - 1) / kRT, 8192)); }
}  // namespace
}  // namespace dgrep
