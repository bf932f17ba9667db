// encode_common.h — the byte-level rules of the three partition writers
// (encode.hip, encode_batch.hip, encode_window.hip): Go's JSON string escaping,
// the key hash step, decimal digits, and the SWAR / realigned-copy helpers. It
// compiles as plain C++ too (tests/escape_c). The pipeline that the resident
// and the batch writer build on these is encode_pipeline.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dgrep {

__host__ __device__ inline uint32_t fnv_step(uint32_t h, uint32_t b) { return (h ^ b) * 16777619u; }

// Go encoding/json string escaping (encode.go encodeState.string, HTML escape
// on, as json.NewEncoder sets it): '"' '\\' get a backslash; \n \r \t their
// short forms; other bytes < 0x20 and < > & become \u00XX; invalid UTF-8 (as
// utf8.DecodeRuneInString: each bad byte on its own) becomes \ufffd;
// U+2028/U+2029 become \u2028 / \u2029; every other byte passes unchanged.
// OUT = nullptr measures. Returns the bytes written (quotes excluded).
template <bool WRITE>
__host__ __device__ inline uint64_t json_body(const uint8_t* s, uint64_t n, uint8_t* out) {
  const char* hex = "0123456789abcdef";
  uint64_t o = 0, i = 0;
  auto put = [&](uint8_t ch) {
    if (WRITE) out[o] = ch;
    ++o;
  };
  while (i < n) {
    const uint32_t b = s[i];
    if (b < 0x80) {
      if (b >= 0x20 && b != '"' && b != '\\' && b != '<' && b != '>' && b != '&') {
        put(uint8_t(b));
      } else {
        put('\\');
        if (b == '\\' || b == '"') put(uint8_t(b));
        else if (b == '\n') put('n');
        else if (b == '\r') put('r');
        else if (b == '\t') put('t');
        else { put('u'); put('0'); put('0'); put(uint8_t(hex[b >> 4])); put(uint8_t(hex[b & 15])); }
      }
      ++i;
      continue;
    }
    uint32_t need = 0, lo = 0x80, hi = 0xBF, r = 0;
    bool ok = true;
    if (b >= 0xC2 && b <= 0xDF) { need = 2; r = b & 0x1F; }
    else if (b >= 0xE0 && b <= 0xEF) { need = 3; r = b & 0x0F; if (b == 0xE0) lo = 0xA0; if (b == 0xED) hi = 0x9F; }
    else if (b >= 0xF0 && b <= 0xF4) { need = 4; r = b & 7; if (b == 0xF0) lo = 0x90; if (b == 0xF4) hi = 0x8F; }
    else ok = false;
    if (ok && i + need > n) ok = false;
    if (ok && (s[i + 1] < lo || s[i + 1] > hi)) ok = false;
    for (uint32_t k = 1; ok && k < need; ++k) {
      if (k > 1 && (s[i + k] < 0x80 || s[i + k] > 0xBF)) ok = false;
      r = (r << 6) | (s[i + k] & 0x3Fu);
    }
    if (!ok) {
      put('\\'); put('u'); put('f'); put('f'); put('f'); put('d');
      ++i;
      continue;
    }
    if (r == 0x2028 || r == 0x2029) {
      put('\\'); put('u'); put('2'); put('0'); put('2'); put(uint8_t(hex[r & 15]));
    } else {
      for (uint32_t k = 0; k < need; ++k) put(s[i + k]);
    }
    i += need;
  }
  return o;
}

// {"Key":" + name + " (line number #" + digits + ")" + ,"Value":" + value + "}\n
constexpr uint32_t kFixedBytes = 8 + 15 + 2 + 10 + 3;

#if defined(__HIPCC__)
// bit 7 of byte k set iff byte k of x is zero (exact)
__device__ __forceinline__ uint32_t zero_bytes(uint32_t x) { return ~(((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x) & 0x80808080u; }
// bit 7 of byte k set iff byte k of x needs JSON escaping or is not ASCII:
// < 0x20, >= 0x80, '"', '\\', '<', '>', '&'
__device__ __forceinline__ uint32_t special_bytes(uint32_t x) {
  return zero_bytes(x & 0xe0e0e0e0u) | (x & 0x80808080u) | zero_bytes(x ^ 0x22222222u) | zero_bytes(x ^ 0x5c5c5c5cu) |
         zero_bytes(x ^ 0x3c3c3c3cu) | zero_bytes(x ^ 0x3e3e3e3eu) | zero_bytes(x ^ 0x26262626u);
}
// byte mask (bit 7 of each byte) of the bytes at absolute positions [lo, hi)
// within the aligned word at position w
__device__ __forceinline__ uint32_t range_mask(uint64_t w, uint64_t lo, uint64_t hi) {
  uint32_t m = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (w + uint64_t(k) >= lo && w + uint64_t(k) < hi) m |= 0x80u << (8 * k);
  return m;
}

// dst[0:L) = src[0:L) with 4-byte stores after the head: the source is read in
// aligned dwords and realigned with v_alignbyte (whole-dword reads never pass
// the source's last dword, which lies inside the 16-B-aligned split).
__device__ __forceinline__ void copy_bytes(uint8_t* dst, const uint8_t* src, uint64_t L) {
  uint64_t i = 0;
  while (i < L && (reinterpret_cast<uintptr_t>(dst + i) & 3)) {
    dst[i] = src[i];
    ++i;
  }
  if (L - i >= 8) {
    const uint8_t* s = src + i;
    const uint32_t sh = uint32_t(reinterpret_cast<uintptr_t>(s) & 3);
    const uint32_t* sw = reinterpret_cast<const uint32_t*>(s - sh);
    uint32_t* dw = reinterpret_cast<uint32_t*>(dst + i);
    const uint64_t nd = (L - i) / 4 - 1;  // the last dword needs sw[k + 1], which may lie past the value: leave it
    uint32_t lo = sw[0];
    for (uint64_t k = 0; k < nd; ++k) {
      const uint32_t hi = sw[k + 1];
      // v_alignbyte_b32 takes the shift in BYTES: ({hi, lo} >> 8 * sh)[31:0]
      dw[k] = __builtin_amdgcn_alignbyte(hi, lo, sh);
      lo = hi;
    }
    i += nd * 4;
  }
  for (; i < L; ++i) dst[i] = src[i];
}

// decimal digits of v (most significant first) into d[20]; returns their count.
// Line numbers below 2^32 (every split under 4 G lines) take the 32-bit path,
// whose division by 10 is a multiply-high (the 64-bit one is a library loop).
__device__ __forceinline__ uint32_t digits_of(uint64_t v, uint8_t (&d)[20]) {
  uint8_t t[20];
  uint32_t nd = 0;
  if (v < (1ull << 32)) {
    uint32_t x = uint32_t(v);
    do { t[nd++] = uint8_t(x % 10u); x /= 10u; } while (x);
  } else {
    do { t[nd++] = uint8_t(v % 10u); v /= 10u; } while (v);
  }
  for (uint32_t k = 0; k < nd; ++k) d[k] = t[nd - 1 - k];
  return nd;
}

__device__ inline void put_str(uint8_t*& o, const char* s) {
  while (*s) *o++ = uint8_t(*s++);
}
#endif  // __HIPCC__

}  // namespace dgrep
