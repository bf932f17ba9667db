// carry_plan.h — the host side of carry_walk (carry.h): how a range is cut into
// chunks, and what the walk needs to know about a DFA beyond its table. Plain
// C++, no HIP: tests/carry_c builds it alone under the sanitizers.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

namespace dgrep {

constexpr uint32_t kCarryGuesses = 4;     // guesses per chunk
constexpr uint32_t kCarryLookback = 256;  // bytes walked before a chunk to form its guesses
constexpr uint64_t kCarryMinChunk = 256;  // >= kCarryLookback, a multiple of 16
constexpr uint64_t kCarryRowsLds = 32 << 10;  // DFA rows up to this many bytes go to LDS in the chunk kernel

struct CarryPlan {
  uint64_t chunk = kCarryMinChunk;  // bytes per chunk: kCarryMinChunk << k
  uint64_t nchunks = 0;             // ceil(m / chunk); 0 for m == 0
};

// The smallest chunk of kCarryMinChunk << k that needs at most max_lanes lanes
// for m bytes: short ranges still spread over many lanes, and the (guess, exit)
// scratch stays below 32 * max_lanes bytes whatever m is.
inline CarryPlan carry_plan(uint64_t m, uint64_t max_lanes) {
  CarryPlan p;
  if (max_lanes == 0) max_lanes = 1;
  while (p.chunk < (uint64_t(1) << 62) && m / p.chunk + (m % p.chunk ? 1 : 0) > max_lanes) p.chunk <<= 1;
  p.nchunks = m / p.chunk + (m % p.chunk ? 1 : 0);
  return p;
}

// The lanes to plan m bytes for. The fix kernel's chain is serial, about 85 ns
// a chunk on its one wave; a lane of the chunk kernel takes about 50 ns a byte
// on LDS rows (two dependent LDS reads), several times that on rows read
// through the caches (measured on MI355X). chunk * 50 ns +
// m / chunk * 85 ns is least near chunk = sqrt(1.6 m): about sqrt(m) lanes, and
// four times as many (a quarter of the chunk) where a byte costs more. With
// 1024 lanes per CU the chain of a 256 MiB fold was 2^18 steps, 22 ms.
inline uint64_t carry_lanes(uint64_t m, uint64_t num_cus, bool rows_in_lds) {
  uint64_t r = 1;
  while (r < (uint64_t(1) << 31) && r * r < m) r <<= 1;  // the power of two at or above sqrt(m)
  if (!rows_in_lds) r <<= 2;
  const uint64_t most = (num_cus ? num_cus : 1) * 1024;
  return r < 64 ? 64 : r > most ? most : r;
}

// guesses [nchunks][kCarryGuesses] then exits [nchunks][kCarryGuesses], u32
inline uint64_t carry_pairs_bytes(const CarryPlan& p) { return p.nchunks * kCarryGuesses * 4 * 2; }

// absorbing[x] = 1 iff every class but nl_class loops at x: the walk of a
// newline-free range stays there whatever follows.
inline std::vector<uint8_t> carry_absorbing(const uint32_t* trans, uint32_t nstates, uint32_t nclasses,
                                            uint32_t nl_class) {
  std::vector<uint8_t> a(nstates, 1);
  for (uint32_t x = 0; x < nstates; ++x)
    for (uint32_t k = 0; k < nclasses; ++k)
      if (k != nl_class && trans[size_t(x) * nclasses + k] != x) {
        a[x] = 0;
        break;
      }
  return a;
}

// The lookback's start states: `start`, then states spread over the ids, never
// an absorbing one and never `start` again while another is left -- a DFA that
// keeps a finite memory of the whole line (a parity, a flag) then has seeds in
// several of its memory classes.
inline void carry_seeds(const std::vector<uint8_t>& absorbing, uint32_t nstates, uint32_t start,
                        uint32_t seed[kCarryGuesses]) {
  for (uint32_t i = 0; i < kCarryGuesses; ++i) seed[i] = start;
  for (uint32_t i = 1; i < kCarryGuesses && nstates > 1; ++i) {
    uint32_t x = uint32_t(uint64_t(i) * nstates / kCarryGuesses) % nstates;
    for (uint32_t t = 0; t < nstates; ++t, x = (x + 1) % nstates) {
      bool taken = absorbing[x] != 0;
      for (uint32_t j = 0; j < i && !taken; ++j) taken = seed[j] == x;
      if (!taken) {
        seed[i] = x;
        break;
      }
    }
  }
}

}  // namespace dgrep
