// carry_plan_test — the carry walk's host side (csrc/kernels/carry_plan.h)
// under ASan + UBSan, with a host restatement of the two kernels on exact-size
// heap buffers: for random DFAs and ranges the guess-and-fix walk, planned by
// carry_plan and seeded by carry_seeds, equals the serial walk whatever the
// guesses are, reads nothing outside [0, m), and stops early only where the
// state is absorbing.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <string>
#include <vector>

#include "carry_plan.h"

using namespace dgrep;

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint32_t rnd(uint32_t n) {
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return uint32_t((rng_state >> 20) % n);
}

#define CHECK(cond)                                                \
  do {                                                             \
    if (!(cond)) {                                                 \
      printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);     \
      exit(1);                                                     \
    }                                                              \
  } while (0)

struct Dfa {
  uint32_t S, K, start, nl;
  std::vector<uint32_t> trans;
  std::vector<uint8_t> cls;  // exactly 256
};

static uint32_t step_range(const Dfa& d, const std::vector<uint8_t>& data, uint64_t b, uint64_t e, uint32_t s) {
  for (uint64_t i = b; i < e; ++i) s = d.trans[size_t(s) * d.K + d.cls[data.at(i)]];
  return s;
}

// the chunk kernel and the fix kernel, one after the other; returns the exit state
static uint32_t guess_and_fix(const Dfa& d, const std::vector<uint8_t>& data, uint32_t entry, uint64_t max_lanes,
                              const std::vector<uint8_t>& absorbing, const uint32_t seed[kCarryGuesses],
                              uint64_t* misses, bool* stopped) {
  const uint64_t m = data.size();
  const CarryPlan p = carry_plan(m, max_lanes);
  CHECK(p.chunk >= kCarryLookback && p.chunk % 16 == 0 && (p.chunk & (p.chunk - 1)) == 0);
  CHECK(p.nchunks <= std::max<uint64_t>(max_lanes, 1) && p.nchunks * p.chunk >= m);
  CHECK(m == 0 ? p.nchunks == 0 : (p.nchunks - 1) * p.chunk < m);
  const uint64_t half = p.chunk / 2;  // the next smaller chunk would have needed too many lanes
  CHECK(p.chunk == kCarryMinChunk || m / half + (m % half ? 1 : 0) > std::max<uint64_t>(max_lanes, 1));
  std::vector<uint32_t> pairs(carry_pairs_bytes(p) / 4);  // exact size: an index past it is an ASan report
  uint32_t* guess = pairs.data();
  uint32_t* exit = pairs.data() + p.nchunks * kCarryGuesses;
  for (uint64_t ch = 0; ch < p.nchunks; ++ch) {
    const uint64_t b = ch * p.chunk, e = std::min(m, b + p.chunk);
    for (uint32_t g = 0; g < kCarryGuesses; ++g) {
      uint32_t s = ch == 0 ? entry : step_range(d, data, b - kCarryLookback, b, seed[g]);
      guess[ch * kCarryGuesses + g] = s;
      exit[ch * kCarryGuesses + g] = step_range(d, data, b, e, s);
    }
  }
  uint32_t st = entry;
  *misses = 0;
  *stopped = false;
  for (uint64_t ch = 0; ch < p.nchunks; ++ch) {
    uint32_t g = 0;
    while (g < kCarryGuesses && guess[ch * kCarryGuesses + g] != st) ++g;
    if (g < kCarryGuesses) {
      st = exit[ch * kCarryGuesses + g];
    } else if (absorbing[st]) {  // tested only where the guesses miss: nothing that follows moves the state
      *stopped = true;
      break;
    } else {
      st = step_range(d, data, ch * p.chunk, std::min(m, (ch + 1) * p.chunk), st);
      ++*misses;
    }
  }
  return st;
}

static Dfa random_dfa(uint32_t S, uint32_t K, bool counter) {
  Dfa d;
  d.S = S;
  d.K = K;
  d.start = rnd(S);
  d.cls.resize(256);
  for (int b = 0; b < 256; ++b) d.cls[b] = uint8_t(rnd(K));
  d.nl = d.cls['\n'];
  for (int b = 0; b < 256; ++b)
    if (b != '\n' && d.cls[b] == d.nl) d.cls[b] = uint8_t((d.nl + 1) % K);
  d.trans.resize(size_t(S) * K);
  for (uint32_t s = 0; s < S; ++s)
    for (uint32_t k = 0; k < K; ++k)
      // counter: one class counts modulo S, every other class stays -- a DFA that never forgets
      d.trans[size_t(s) * K + k] = counter ? (k == (d.nl + 1) % K ? (s + 1) % S : s) : rnd(S);
  return d;
}

// `carry_plan_test print`: what carry_plan.h computes for inputs written out
// here and, the same, in tests/test_carry_plan.py, which compares these lines
// with tests/carry_cases.py's restatement of the four functions.
static const uint64_t kPrintM[] = {0,      1,      255,     256,     257,     4095,    4096,    4097,    16383,
                                   16384,  65535,  65536,   65537,   131071,  131072,  131073,  262143,  262144,
                                   262145, 524289, 1048575, 1048576, 1048577, 2097151, 2097152, 2097153, 268435456,
                                   (uint64_t(1) << 32) + 1, uint64_t(1) << 40};
static const uint64_t kPrintCus[] = {0, 1, 4, 256, 304};

// [nstates][nclasses]; the class of '\n' is 1 in both
static const uint32_t kTableA[6][3] = {{1, 0, 2}, {1, 0, 1}, {2, 5, 2}, {3, 3, 3}, {4, 0, 4}, {0, 1, 2}};
static const uint32_t kTableB[9][2] = {{0, 3}, {1, 1}, {2, 0}, {3, 4}, {5, 0}, {5, 5}, {6, 1}, {7, 2}, {1, 8}};

template <uint32_t S, uint32_t K>
static void print_table(const char* name, const uint32_t (&t)[S][K], uint32_t nl) {
  const std::vector<uint8_t> a = carry_absorbing(&t[0][0], S, K, nl);
  printf("absorbing %s", name);
  for (uint32_t x = 0; x < S; ++x) printf(" %u", unsigned(a[x]));
  printf("\n");
  for (uint32_t start = 0; start < S; ++start) {
    uint32_t seed[kCarryGuesses];
    carry_seeds(a, S, start, seed);
    printf("seeds %s %u: %u %u %u %u\n", name, start, seed[0], seed[1], seed[2], seed[3]);
  }
  // fewer states than guesses: the first n rows as a table of their own (every entry taken modulo n)
  for (uint32_t n = 1; n <= 3; ++n) {
    std::vector<uint32_t> small(size_t(n) * K);
    for (uint32_t x = 0; x < n; ++x)
      for (uint32_t k = 0; k < K; ++k) small[size_t(x) * K + k] = t[x][k] % n;
    const std::vector<uint8_t> sa = carry_absorbing(small.data(), n, K, nl);
    uint32_t seed[kCarryGuesses];
    carry_seeds(sa, n, n - 1, seed);
    printf("small %s %u:", name, n);
    for (uint32_t x = 0; x < n; ++x) printf(" %u", unsigned(sa[x]));
    printf(" : %u %u %u %u\n", seed[0], seed[1], seed[2], seed[3]);
  }
}

static int print_mode() {
  for (uint64_t m : kPrintM)
    for (uint64_t cus : kPrintCus)
      for (int lds = 1; lds >= 0; --lds) {
        const uint64_t lanes = carry_lanes(m, cus, lds != 0);
        const CarryPlan p = carry_plan(m, lanes);
        printf("plan %llu %llu %d: %llu %llu %llu\n", (unsigned long long)m, (unsigned long long)cus, lds,
               (unsigned long long)lanes, (unsigned long long)p.chunk, (unsigned long long)p.nchunks);
      }
  for (uint64_t lanes : {uint64_t(0), uint64_t(1), uint64_t(3), uint64_t(64)}) {
    const CarryPlan p = carry_plan(100000, lanes);
    printf("lanes %llu: %llu %llu\n", (unsigned long long)lanes, (unsigned long long)p.chunk,
           (unsigned long long)p.nchunks);
  }
  print_table("A", kTableA, 1);
  print_table("B", kTableB, 1);
  return 0;
}

int main(int argc, char** argv) {
  if (argc > 1 && std::string(argv[1]) == "print") return print_mode();
  // the plan alone, at sizes no buffer could have
  for (uint64_t m : {uint64_t(0), uint64_t(1), uint64_t(255), uint64_t(256), uint64_t(257), uint64_t(1) << 20,
                     (uint64_t(1) << 41) - 1, ~uint64_t(0) >> 1, ~uint64_t(0)})
    for (uint64_t lanes : {uint64_t(0), uint64_t(1), uint64_t(7), uint64_t(262144)}) {
      const CarryPlan p = carry_plan(m, lanes);
      CHECK(p.chunk >= kCarryMinChunk);
      CHECK(p.nchunks == m / p.chunk + (m % p.chunk ? 1 : 0));
      CHECK(p.chunk == (uint64_t(1) << 62) || p.nchunks <= std::max<uint64_t>(lanes, 1));
      CHECK(carry_pairs_bytes(p) == p.nchunks * 32);
    }
  for (uint64_t m : {uint64_t(0), uint64_t(1), uint64_t(4096), uint64_t(65536), uint64_t(65537), uint64_t(1) << 28,
                     (uint64_t(1) << 29) - 1, uint64_t(1) << 41, ~uint64_t(0)})
    for (uint64_t cus : {uint64_t(0), uint64_t(1), uint64_t(256)})
      for (bool lds : {true, false}) {
        const uint64_t lanes = carry_lanes(m, cus, lds);
        CHECK(lanes >= 64 && lanes <= std::max<uint64_t>(std::max<uint64_t>(cus, 1) * 1024, 64));
        const CarryPlan p = carry_plan(m, lanes);
        CHECK(p.nchunks <= lanes || p.chunk == (uint64_t(1) << 62));
        if (m <= 65536) CHECK(p.chunk == kCarryMinChunk);  // short ranges keep the smallest chunk
      }
  uint64_t total_misses = 0, total_stops = 0, walks = 0;
  for (int round = 0; round < 100; ++round) {
    const bool counter = round % 3 == 0;
    const uint32_t S = counter ? 2 + rnd(9) : 1 + rnd(40), K = 2 + rnd(6);
    Dfa d = random_dfa(S, K, counter);
    if (round % 5 == 1) {  // an absorbing state the walk can fall into
      const uint32_t a = rnd(S);
      for (uint32_t k = 0; k < K; ++k)
        if (k != d.nl) d.trans[size_t(a) * K + k] = a;
    }
    const std::vector<uint8_t> absorbing = carry_absorbing(d.trans.data(), S, K, d.nl);
    CHECK(absorbing.size() == S);
    for (uint32_t s = 0; s < S; ++s) {
      bool loops = true;
      for (uint32_t k = 0; k < K; ++k) loops = loops && (k == d.nl || d.trans[size_t(s) * K + k] == s);
      CHECK(loops == (absorbing[s] != 0));
    }
    uint32_t seed[kCarryGuesses];
    carry_seeds(absorbing, S, d.start, seed);
    CHECK(seed[0] == d.start);
    for (uint32_t i = 0; i < kCarryGuesses; ++i) {
      CHECK(seed[i] < S);
      CHECK(seed[i] == d.start || !absorbing[seed[i]]);
      for (uint32_t j = 1; j < i; ++j) CHECK(seed[i] == d.start || seed[i] != seed[j]);
    }
    for (uint64_t m : {uint64_t(0), uint64_t(1), uint64_t(15), uint64_t(256), uint64_t(257), uint64_t(511),
                       uint64_t(4096), uint64_t(5000 + rnd(3000)), uint64_t(70000 + rnd(999))}) {
      std::vector<uint8_t> data(m);  // exact size
      for (auto& b : data) {
        b = uint8_t(rnd(256));
        if (b == '\n') b = 'x';
      }
      for (uint64_t lanes : {uint64_t(1), uint64_t(3), uint64_t(16), uint64_t(1) << 18}) {
        const uint32_t entry = rnd(S);
        uint64_t misses = 0;
        bool stopped = false;
        const uint32_t got = guess_and_fix(d, data, entry, lanes, absorbing, seed, &misses, &stopped);
        const uint32_t want = step_range(d, data, 0, m, entry);
        CHECK(got == want);
        CHECK(!stopped || absorbing[want]);
        total_misses += misses;
        total_stops += stopped;
        ++walks;
      }
    }
  }
  CHECK(total_misses > 0 && total_stops > 0);
  printf("carry_plan OK: %llu walks, %llu misses, %llu early stops\n", (unsigned long long)walks,
         (unsigned long long)total_misses, (unsigned long long)total_stops);
  return 0;
}
