// carry.h — the DFA state of an unfinished line carried across windows
// (carry.hip), shared with the runtime.
//
// The blob's DFA restarts only at '\n' (include/dgrep_blob.h), so a line that
// outgrows a window needs only its current state kept, not its bytes: a line
// matches iff trans[state at its end][class('\n')] == start_m. carry_walk takes
// a newline-free byte range and an entry state and leaves the exit state, in
// parallel and exactly for any DFA: guess and fix, as the parked filter lines
// (DESIGN 3.7), restated for an arbitrary entry state.
//
//   chunk kernel  one lane per chunk. Chunk 0 starts from the true entry state;
//                 every other chunk walks the kLookback bytes before it from
//                 kGuesses seed states and keeps what they reach as its
//                 guesses, then walks the chunk from each guess and stores the
//                 (guess, exit) pairs.
//   fix kernel    one wave follows the chunk chain from the true entry state:
//                 the stored exit where the state is among a chunk's guesses,
//                 else the chunk walked again from the true state (a miss) --
//                 unless the state is absorbing, where it stops.
//
// The result does not depend on the guesses; only the time does. None of these
// kernels touches the scan kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "carry_plan.h"

namespace dgrep {

// The plain DFA on the device, in the blob's own state ids.
struct CarryTable {
  const void* trans = nullptr;      // [nstates][nclasses]: u16 while ids fit, u32 above 65535 states
  const uint8_t* cls = nullptr;     // [256]
  const uint8_t* absorbing = nullptr;  // [nstates]: every class but '\n' loops
  uint32_t nstates = 0, nclasses = 0;
  uint32_t start = 0, start_m = 0, nl_class = 0;
  uint32_t seed[kCarryGuesses] = {0, 0, 0, 0};  // the lookback's start states; seed[0] = start
  bool u32 = false;
};

struct CarryWalk {
  const uint8_t* data = nullptr;  // 16-byte aligned; the allocation covers m rounded up to 16 bytes
  uint64_t m = 0;                 // data[0 : m) holds no '\n'; may be 0
  // The entry state: `start` if from_start, else *state. *state = the exit
  // state afterwards (device memory, so the next walk needs no host round trip).
  uint32_t* state = nullptr;
  bool from_start = false;
  // verdict[0] = trans[exit][class('\n')] == start_m, if not null. With `dual`
  // the same range is also walked from `start` and verdict[1] is that walk's
  // verdict: what an ordinary scan makes of the range as a line of its own.
  uint32_t* verdict = nullptr;
  bool dual = false;
  uint32_t* pairs = nullptr;            // scratch: carry_pairs_bytes(plan) bytes
  unsigned long long* counters = nullptr;  // [0] += chunks, [1] += guess misses
};

// Queued on s; no host synchronisation.
hipError_t carry_walk(const CarryTable& t, const CarryWalk& w, const CarryPlan& plan, hipStream_t s);

// dst_*[0] = one record (the carried line's, in the stream's coordinates)
hipError_t carry_put_record(uint64_t* dst_line, uint64_t* dst_start, uint64_t* dst_len, uint64_t line_no,
                            uint64_t start, uint64_t len, hipStream_t s);

}  // namespace dgrep
