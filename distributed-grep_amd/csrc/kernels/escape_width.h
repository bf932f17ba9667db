// escape_width.h — Go's JSON string escaping (encode_common.h, json_body) as a
// LOCAL rule: how many bytes byte i of a value becomes, and which, from bytes
// i-3 .. i+3 alone. json_body walks a value front to back; this form lets any
// number of lanes take any bytes of it.
//
// Why it is local: a lead byte (0xC2..0xF4) is never a continuation byte
// (0x80..0xBF), so no sequence ever swallows one, and json_body reaches every
// lead as the start of a step. Whether the lead at j starts a valid sequence
// depends on bytes j..j+3 and on j + need <= L only; byte i is swallowed iff a
// valid sequence starts at one of i-3..i-1 and reaches i. Widths:
//   plain ASCII 1; '"' '\\' \n \r \t 2; other controls, < > & 6; a valid lead
//   its sequence's length (E2 80 A8 / E2 80 A9: 6); a swallowed continuation 0;
//   any other byte >= 0x80 6 (the replacement rune, written �).
// Host and device: the host side is tests/escape_c.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define DGREP_HD __host__ __device__
#else
#define DGREP_HD
#endif

namespace dgrep {

// Length (2..4) of the valid UTF-8 sequence that starts with b0 b1 b2 b3, of
// which `after` bytes behind b0 lie inside the value; 0 if there is none.
// json_body's rules: the second byte's range after E0, ED, F0 and F4.
DGREP_HD inline uint32_t utf8_seq_len(uint32_t b0, uint32_t b1, uint32_t b2, uint32_t b3, uint32_t after) {
  uint32_t need, lo = 0x80, hi = 0xBF;
  if (b0 >= 0xC2 && b0 <= 0xDF) need = 2;
  else if (b0 >= 0xE0 && b0 <= 0xEF) { need = 3; if (b0 == 0xE0) lo = 0xA0; if (b0 == 0xED) hi = 0x9F; }
  else if (b0 >= 0xF0 && b0 <= 0xF4) { need = 4; if (b0 == 0xF0) lo = 0x90; if (b0 == 0xF4) hi = 0x8F; }
  else return 0;
  if (need - 1 > after) return 0;  // i + need <= L, counted within the value
  if (b1 < lo || b1 > hi) return 0;
  if (need >= 3 && (b2 < 0x80 || b2 > 0xBF)) return 0;
  if (need >= 4 && (b3 < 0x80 || b3 > 0xBF)) return 0;
  return need;
}

// w[0..6] = bytes i-3 .. i+3 of the value (w[3] is byte i); `before` = min(i, 3)
// and `after` = min(L - 1 - i, 3) say how many of them lie inside the value;
// the others are never looked at.
DGREP_HD inline uint32_t escape_width(const uint8_t* w, uint32_t before, uint32_t after) {
  const uint32_t b = w[3];
  if (b < 0x80) {
    if (b >= 0x20 && b != '"' && b != '\\' && b != '<' && b != '>' && b != '&') return 1;
    return (b == '"' || b == '\\' || b == '\n' || b == '\r' || b == '\t') ? 2 : 6;
  }
  if (b <= 0xBF) {  // a continuation byte: swallowed by a sequence that starts up to 3 bytes before?
    if (before >= 1 && utf8_seq_len(w[2], w[3], w[4], w[5], after + 1) > 1) return 0;
    if (before >= 2 && utf8_seq_len(w[1], w[2], w[3], w[4], after + 2) > 2) return 0;
    if (before >= 3 && utf8_seq_len(w[0], w[1], w[2], w[3], after + 3) > 3) return 0;
    return 6;
  }
  const uint32_t need = utf8_seq_len(b, w[4], w[5], w[6], after);
  if (need == 0) return 6;
  if (need == 3 && b == 0xE2 && w[4] == 0x80 && (w[5] == 0xA8 || w[5] == 0xA9)) return 6;  // U+2028 / U+2029
  return need;
}

// The `width` bytes byte i becomes (width = escape_width of the same window), to out[0 : width).
DGREP_HD inline void escape_put(const uint8_t* w, uint32_t after, uint32_t width, uint8_t* out) {
  const char* hex = "0123456789abcdef";
  const uint32_t b = w[3];
  if (width == 0) return;
  if (b < 0x80) {
    if (width == 1) { out[0] = uint8_t(b); return; }
    out[0] = '\\';
    if (width == 2) {
      out[1] = b == '\n' ? 'n' : b == '\r' ? 'r' : b == '\t' ? 't' : uint8_t(b);
      return;
    }
    out[1] = 'u'; out[2] = '0'; out[3] = '0';
    out[4] = uint8_t(hex[b >> 4]);
    out[5] = uint8_t(hex[b & 15]);
    return;
  }
  if (width == 6) {
    out[0] = '\\'; out[1] = 'u';
    if (after >= 2 && b == 0xE2 && w[4] == 0x80 && (w[5] == 0xA8 || w[5] == 0xA9)) {  // whole inside the value: valid
      out[2] = '2'; out[3] = '0'; out[4] = '2';
      out[5] = uint8_t(hex[w[5] & 15]);
    } else {
      out[2] = 'f'; out[3] = 'f'; out[4] = 'f'; out[5] = 'd';
    }
    return;
  }
  out[0] = w[3];  // a valid sequence of 2..4 bytes, unchanged
  out[1] = w[4];
  if (width > 2) out[2] = w[5];
  if (width > 3) out[3] = w[6];
}

// Host / one-thread form over a whole value: byte i's window, clipped to [0, L).
// The slots outside the value get a continuation byte, the worst a kernel can
// find there (another line's bytes, or what an earlier window left in the
// buffer): a rule that looked at them would take a truncated sequence for whole.
DGREP_HD inline uint32_t escape_width_at(const uint8_t* s, uint64_t L, uint64_t i, uint8_t* w /* [7] */) {
  const uint32_t before = uint32_t(i < 3 ? i : 3), after = uint32_t(L - 1 - i < 3 ? L - 1 - i : 3);
  for (uint32_t k = 0; k < 7; ++k) w[k] = 0x80;
  for (uint32_t k = 0; k <= before; ++k) w[3 - k] = s[i - k];
  for (uint32_t k = 1; k <= after; ++k) w[3 + k] = s[i + k];
  return escape_width(w, before, after);
}

}  // namespace dgrep
