// fnv64_collide.cpp — find different keys with the same FNV-1a 64 hash.
//
// The reduce groups lines by the FNV-1a 64 of the decoded key and settles
// equal hashes with an exact compare (csrc/kernels/reduce.hip dedupe_kernel,
// reduce_batch.hip dedupe_batch_kernel). This program makes the inputs that
// reach the compare's "different" verdicts: the pairs in
// tests/golden/fnv64_collisions.json. It is a host-only tool and no test runs
// it; tests/test_fnv64_collisions.py re-verifies every pair it ever printed.
//
//   g++ -O2 -std=c++17 -pthread tools/fnv64_collide.cpp -o fnv64_collide
//
//   fnv64_collide                         one pair of 11-byte keys from the offset basis
//   fnv64_collide --state 0xc90a3dfcaa12b417
//                                         a pair that collides when hashed FROM that state:
//                                         appended to both keys of an earlier pair it gives
//                                         four keys with one hash (chain again for eight)
//   fnv64_collide --prefix STRING         the same, the state being STRING's hash: the
//                                         pair first differs at byte len(STRING)
//   fnv64_collide --len 11 --len2 12      keys of either length; only a pair of one
//                                         11-byte and one 12-byte key is accepted
//   --pairs N     stop after N pairs (default 1)
//   --threads T   default min(16, hardware threads)
//   --dp-bits D   a trail ends at a value whose D middle bits are zero (default 16)
//   --seed S      other start points, hence other pairs
//
// The default initial state is the reduce's own constant (reduce_common.h
// json_string, 1469598103934665603): the collisions are collisions of THAT hash.
//
// Method: the parallel distinguished-point search of van Oorschot and Wiener.
// f(x) = FNV-1a 64, from the initial state, of key(x); key(x) spells the low
// bits of x five at a time over the alphabet a-z0-5 (no byte of it needs a JSON
// escape). Every thread walks x -> f(x) from random starts and stores
// (end -> start, steps) for trails that end in a distinguished value. Two
// trails with the same end have merged: walking both again, in step, finds a
// and b with f(a) == f(b), a != b. Where key(a) == key(b) (x has more bits than
// a short key spells: 55 for 11 bytes) that is no collision of keys and is
// skipped; about one merge in 2^(64 - 5 len) is a real one.
// Expected work: about 2^32 to 2^33 hash evaluations per pair whatever the
// length (a 64-bit birthday), i.e. seconds to a few minutes on 8-16 threads;
// the mixed-length mode discards the equal-length half and takes about 1.5x.
// Each result line is `keyA keyB 0x<common hash>`; with --prefix the keys are
// printed with the prefix in front. Statistics go to stderr.
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

namespace {
constexpr uint64_t kBasis = 1469598103934665603ull, kPrime = 1099511628211ull;
constexpr int kMaxLen = 24;
const char kAlphabet[33] = "abcdefghijklmnopqrstuvwxyz012345";

struct Params {
  uint64_t state = kBasis;
  int len = 11, len2 = 0;  // len2 != 0: bit 63 of x picks the length
  int dp_bits = 16;
};

inline uint64_t fnv(uint64_t h, const char* s, size_t n) {
  for (size_t i = 0; i < n; ++i) h = (h ^ uint8_t(s[i])) * kPrime;
  return h;
}

// key(x): out has room for kMaxLen bytes; bits past bit 63 read as zero
inline int key_of(const Params& p, uint64_t x, char* out) {
  const int len = p.len2 && (x >> 63) ? p.len2 : p.len;
  for (int i = 0; i < len; ++i) out[i] = kAlphabet[5 * i < 64 ? (x >> (5 * i)) & 31u : 0u];
  return len;
}

inline uint64_t step(const Params& p, uint64_t x) {
  char k[kMaxLen];
  const int len = key_of(p, x, k);
  return fnv(p.state, k, size_t(len));
}

inline bool distinguished(const Params& p, uint64_t x) { return ((x >> 24) & ((uint64_t(1) << p.dp_bits) - 1)) == 0; }

struct Trail {
  uint64_t start, steps;
};

// Trails a and b end in the same value. The two values just before they meet,
// or false if one trail runs into the other's start (no collision there).
bool locate(const Params& p, Trail a, Trail b, uint64_t* xa, uint64_t* xb, uint64_t* evals) {
  uint64_t x = a.start, y = b.start;
  for (; a.steps > b.steps; --a.steps, ++*evals) x = step(p, x);
  for (; b.steps > a.steps; --b.steps, ++*evals) y = step(p, y);
  if (x == y) return false;
  for (uint64_t left = a.steps; left > 0; --left) {
    const uint64_t nx = step(p, x), ny = step(p, y);
    *evals += 2;
    if (nx == ny) {
      *xa = x;
      *xb = y;
      return true;
    }
    x = nx;
    y = ny;
  }
  return false;
}

uint64_t splitmix(uint64_t* s) {
  uint64_t z = (*s += 0x9e3779b97f4a7c15ull);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}

[[noreturn]] void usage(const char* why) {
  std::fprintf(stderr,
               "fnv64_collide: %s\nusage: fnv64_collide [--state HEX | --prefix STRING] [--len L] [--len2 L2] "
               "[--pairs N] [--threads T] [--dp-bits D] [--seed S]\n",
               why);
  std::exit(2);
}
}  // namespace

int main(int argc, char** argv) {
  Params p;
  std::string prefix;
  bool have_state = false;
  int pairs = 1;
  unsigned hw = std::thread::hardware_concurrency();
  int threads = int(hw == 0 ? 1 : hw > 16 ? 16 : hw);
  uint64_t seed = 1;
  for (int i = 1; i < argc; ++i) {
    const std::string a = argv[i];
    auto val = [&]() -> const char* {
      if (i + 1 >= argc) usage(("missing value after " + a).c_str());
      return argv[++i];
    };
    if (a == "--state") { p.state = std::strtoull(val(), nullptr, 16); have_state = true; }
    else if (a == "--prefix") prefix = val();
    else if (a == "--len") p.len = std::atoi(val());
    else if (a == "--len2") p.len2 = std::atoi(val());
    else if (a == "--pairs") pairs = std::atoi(val());
    else if (a == "--threads") threads = std::atoi(val());
    else if (a == "--dp-bits") p.dp_bits = std::atoi(val());
    else if (a == "--seed") seed = std::strtoull(val(), nullptr, 0);
    else usage(("unknown option " + a).c_str());
  }
  if (have_state && !prefix.empty()) usage("--state and --prefix exclude each other");
  if (p.len < 1 || p.len > kMaxLen || p.len2 < 0 || p.len2 > kMaxLen) usage("key lengths are 1..24");
  if (p.len2 == p.len) usage("--len2 must differ from --len");
  if (p.dp_bits < 1 || p.dp_bits > 30) usage("--dp-bits is 1..30");
  if (threads < 1 || threads > 256 || pairs < 1) usage("bad --threads or --pairs");
  if (!prefix.empty()) p.state = fnv(kBasis, prefix.data(), prefix.size());

  std::mutex mu;  // guards seen, found and the printing
  std::unordered_map<uint64_t, Trail> seen;
  int found = 0;
  uint64_t merges = 0, same_key = 0, same_len = 0;
  std::atomic<bool> done{false};
  std::atomic<uint64_t> evals{0};
  const auto t0 = std::chrono::steady_clock::now();

  auto worker = [&](int t) {
    // (a stream of its own per thread: splitmix steps by a constant, so seeds that differ by a multiple of it overlap)
    uint64_t mix = seed ^ p.state, rng = splitmix(&mix) ^ (uint64_t(t + 1) << 56) ^ uint64_t(t) * 0xd1342543de82ef95ull;
    rng = splitmix(&rng);
    const uint64_t give_up = uint64_t(20) << p.dp_bits;  // a trail caught in a cycle without a distinguished value
    while (!done.load(std::memory_order_relaxed)) {
      Trail mine{splitmix(&rng), 0};
      uint64_t x = mine.start;
      while (!distinguished(p, x) && mine.steps < give_up) {
        x = step(p, x);
        ++mine.steps;
      }
      uint64_t local = mine.steps;
      Trail other{};
      bool merged = false;
      if (distinguished(p, x) && mine.steps > 0) {
        std::lock_guard<std::mutex> lk(mu);
        auto it = seen.find(x);
        if (it == seen.end()) seen.emplace(x, mine);
        else if (it->second.start != mine.start) { other = it->second; merged = true; }
      }
      uint64_t xa, xb;
      if (merged && locate(p, other, mine, &xa, &xb, &local)) {
        char ka[kMaxLen], kb[kMaxLen];
        const int na = key_of(p, xa, ka), nb = key_of(p, xb, kb);
        std::lock_guard<std::mutex> lk(mu);
        ++merges;
        if (na == nb && std::memcmp(ka, kb, size_t(na)) == 0) ++same_key;  // two values, one key: not a result
        else if (p.len2 && na == nb) ++same_len;
        else if (!done.load()) {
          const uint64_t h = fnv(p.state, ka, size_t(na));
          if (h != fnv(p.state, kb, size_t(nb))) { std::fprintf(stderr, "internal error: no collision\n"); std::exit(1); }
          std::printf("%s%.*s %s%.*s 0x%016llx\n", prefix.c_str(), na, ka, prefix.c_str(), nb, kb,
                      (unsigned long long)h);
          std::fflush(stdout);
          if (++found >= pairs) done.store(true);
        }
      }
      evals.fetch_add(local, std::memory_order_relaxed);
    }
  };
  std::vector<std::thread> pool;
  for (int t = 0; t < threads; ++t) pool.emplace_back(worker, t);
  for (auto& th : pool) th.join();
  const double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  std::fprintf(stderr,
               "state 0x%016llx len %d%s%s: %d pair(s), %.1f s on %d threads, 2^%.2f evaluations, %zu trails, "
               "%llu merges (%llu of one key, %llu of one length)\n",
               (unsigned long long)p.state, p.len, p.len2 ? "/" : "", p.len2 ? std::to_string(p.len2).c_str() : "",
               found, secs, threads, std::log2(double(evals.load()) + 1), seen.size(), (unsigned long long)merges,
               (unsigned long long)same_key, (unsigned long long)same_len);
  return 0;
}
