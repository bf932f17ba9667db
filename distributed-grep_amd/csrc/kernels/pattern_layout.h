// pattern_layout.h — the constants that define a loaded pattern's images.
//
// Plain C++ with no HIP in it. scan_common.h includes it and adds the pair
// stepper's limits (kPair*), which stay there beside the kernels' argument
// structs; both headers compile as plain C++, so the host-only image builder
// (runtime/pattern_image.h) and its stand-alone driver (tests/pattern_image_c)
// read the same names as the kernels.
#pragma once
#include <stdint.h>

// DFAs of at most this many states use the Sheng stepper (8 = its limit; 0
// sends every DFA of <= 256 states to the table stepper)
#ifndef DGREP_SHENG_MAX_STATES
#define DGREP_SHENG_MAX_STATES 8
#endif
// DFAs above the Sheng limit whose two-byte table fits in LDS use the pair
// stepper (0: they use the u8 table stepper)
#ifndef DGREP_PAIR_ENABLE
#define DGREP_PAIR_ENABLE 1
#endif
// the filter image's row pitch: see build_filter_image (0: the class count)
#ifndef DGREP_FILTER_PITCH
#define DGREP_FILTER_PITCH 1
#endif

namespace dgrep {

// DFA stepper selected by build_pattern_image from the state count.
enum : int {
  kStepTable = 0,   // <= 256 states: u8 [state][byte] table, 260-byte rows
  kStepSheng8 = 1,  // <= 8 states: per-byte 8-state vectors (v_perm stepping)
  // 2: the r01 wide stepper (u16 rows, cold ones from HBM on the chain), removed in round 6
  kStepPair = 3,    // 2 * states * classes^2 <= kPairMaxT2 bytes: two input bytes per table lookup
  kStepFilter = 4,  // > 256 states: the DFA's shallow part in LDS, lines that leave it verified afterwards
  // 5: the r05 word stepper (one lookup per 4-byte word), measured slower than pair; removed in round 6
};

// StepTable's row stride: 256 entries and one dword, so that the rows are
// bank-staggered
constexpr uint32_t kTableRow = 260;

// LDS image of kStepFilter: byte classes [256] (u8), then u16 [state][class]
// rows of the filter DFA (its states premultiplied by the class count), at
// most this many bytes in all -- with 1024 threads x 4 slots x 8 B the
// workgroup stays within the CU's 160 KiB.
#ifndef DGREP_FILTER_KIB
#define DGREP_FILTER_KIB 124
#endif
constexpr uint32_t kFilterImageBytes = DGREP_FILTER_KIB * 1024;
// u8 classes: four byte values share a dword, so printable ASCII (0x20-0x7f)
// spans 24 dwords in 24 distinct banks and a wave's class reads of text never
// conflict (tools/lds_bank_bench.hip on the log corpus: u8 table 0 % conflict
// cycles, u32 entries at 4*b 52 %, u64 at 8*b 55 %). C4 kernel 3.18 -> 3.38 TB/s.
constexpr uint32_t kFilterClassBytes = 256;

// StepPair image offsets and thresholds (see StepPair in scan_dfa.hip)
struct PairArgs {
  uint32_t t1 = 0, thr = 0, div = 0, w32 = 0;
};

// verify_kernel: leading bytes of the whole DFA's rows that each 256-thread
// workgroup copies to LDS (the rest are read from HBM)
constexpr uint32_t kVerifyHotBytes = 48 * 1024;
// long_dfa_seg1_kernel: one 1024-thread workgroup per CU holds this much of
// the whole DFA in LDS
constexpr uint32_t kLongDfaHotBytes = 120 * 1024;  // rows alone (u32 DFAs)
constexpr uint32_t kLongDfaLdsBytes = 158 * 1024;  // rows + DfaXRec (u16 DFAs)
// start states of a long line's lookback (LongDfaArgs::seed)
constexpr int kLongSeeds = 8;

// DfaXRec: a state past the LDS image's first rows reads the row of a resident
// DEFAULT state except in at most two classes (keyword automata: 4,608 of
// config 4's 4,978 such states differ in one class, 367 in two; the 2 left
// get an extra row of their own as default): x = default row | class 1 << 16
// | class 2 << 24 (0xff: unused), y = next state on class 1 | on class 2 << 16.
// The kernels read a record as one uint2.
constexpr uint32_t kXNone = 0xffu;
struct DfaXRec {
  uint32_t x, y;
};

}  // namespace dgrep
