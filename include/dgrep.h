/*
 * dgrep.h — C ABI of libdgrep.so, the MI355X-native Map hot path of
 * distributed-grep (bgilby59/distributed-grep).
 *
 * The reference path being replaced is the body of the grep plugin's Map:
 *
 *   application/grep.go:13-36
 *     lines := strings.Split(contents, "\n")                 // grep.go:17
 *     for line_number, line := range lines {                 // grep.go:20
 *         matched, _ := regexp.Match(pattern, []byte(line))  // grep.go:21
 *         if matched {                                       // grep.go:24-29
 *             k := fmt.Sprintf("%s (line number #%v)", filename, line_number+1)
 *             kva = append(kva, KeyValue{Key: k, Value: line})
 *
 * A cgo-built Map binds exactly these entry points: it
 * compiles `pattern` once (dgrep_compile -> dgrep_load_dfa, replacing the
 * per-line regexp.Compile inside regexp.Match at grep.go:21), scans the split
 * on the GPU (dgrep_scan, replacing grep.go:17-24), and rebuilds each
 * KeyValue on the host from (line_no, start, len): Key = Sprintf(filename,
 * line_no), Value = contents[start:start+len] (grep.go:25-28). Reduce
 * (grep.go:38-40) is unchanged.
 *
 * Conventions: every function returns an int status (DGREP_OK = 0). The
 * library borrows `data` only for the duration of a call; result arrays are
 * owned by the library until dgrep_result_free. Each entry point sets the
 * context's HIP device, so a Go goroutine may migrate between OS threads.
 * One context per device stream; contexts share no mutable state.
 */
#ifndef DGREP_H
#define DGREP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum {
  DGREP_OK = 0,
  DGREP_E_INVALID = 1,     /* bad argument / malformed blob */
  DGREP_E_UNSUPPORTED = 2, /* valid Go regexp outside the compiler's subset: refuse, never guess */
  DGREP_E_TOO_LARGE = 3,   /* DFA over the state budget AND its NFA over DGREP_NFA_MAX_POS (8192) positions */
  DGREP_E_HIP = 4,         /* HIP runtime error (message in dgrep_last_error) */
  DGREP_E_NOMEM = 5,
  DGREP_E_NO_DFA = 6,      /* scan before dgrep_load_dfa */
};

/* Flags carried in a compiled blob (dgrep_blob_info). */
enum {
  DGREP_DFA_GO_SYNTAX_ERROR = 1u << 0, /* Go's regexp.Compile rejects the pattern: no line matches (grep.go:21 drops err) */
  DGREP_DFA_MATCH_NONE = 1u << 1,      /* no line can match */
  DGREP_DFA_MATCH_ALL = 1u << 2,       /* every line matches (e.g. the shipped pattern "" at grep.go:11) */
  DGREP_DFA_PARTIAL = 1u << 3,         /* DFA beyond the state budget: first states + CAND + NFA program (dgrep_blob.h) */
};

typedef struct dgrep_ctx dgrep_ctx;

/* Matching lines of one split, ascending line order (grep.go:20 iteration
 * order). line_no is 1-based (grep.go:25 `line_number+1`); start/len index
 * the split's bytes; the line excludes its '\n' (strings.Split). len is 64-bit:
 * a Go string (and so a line of one) may be longer than 4 GiB. */
typedef struct {
  uint64_t count;
  uint64_t* line_no;
  uint64_t* start;
  uint64_t* len;
} dgrep_result;

typedef struct {
  uint32_t flags;
  uint32_t nstates;  /* minimized DFA states */
  uint32_t nclasses; /* byte equivalence classes */
  uint32_t start;
  uint32_t start_m;  /* the state entered by a '\n' that ends a matching line */
} dgrep_blob_info;

/* ---- pattern compiler (host only, no GPU needed) ------------------------ */
/* Replaces regexp.Compile(pattern) inside regexp.Match (grep.go:21) with Go
 * regexp/syntax Perl-flag semantics. A pattern Go rejects still returns
 * DGREP_OK with a blob flagged DGREP_DFA_GO_SYNTAX_ERROR|MATCH_NONE, because
 * the reference discards the error and matches nothing. `err` (optional)
 * receives a message for non-OK results. */
int dgrep_compile(const char* pattern, size_t n, void** blob, size_t* blob_len, char* err, size_t errlen);
/* Tests only: dgrep_compile with the DFA state budget lowered to state_budget
 * (0 = the default 2^21; values below 3 are ignored), so that the partial-blob
 * path (DGREP_DFA_PARTIAL) can be exercised with small patterns. */
int dgrep_compile_budget(const char* pattern, size_t n, uint32_t state_budget, void** blob, size_t* blob_len,
                         char* err, size_t errlen);
void dgrep_blob_free(void* blob);
/* Validates the whole blob (header, byte classes, every transition, and the
 * NFA program of a partial blob word by word) before reporting its header:
 * DGREP_E_INVALID if anything would index out of range. dgrep_load_dfa
 * calls it first. */
int dgrep_blob_info_get(const void* blob, size_t n, dgrep_blob_info* info);

/* ---- device context ------------------------------------------------------ */
/* The worker's device (map_reduce/worker.go:126-145 runs one map task at a
 * time per worker process, one file per task, coordinator.go:312,329-333): the
 * DGREP_DEVICE environment variable if set, else worker_id % device_count, where
 * a negative worker_id means the DGREP_WORKER_ID environment variable, else the
 * process id (the Go plugin has no worker id: WorkerID stays inside the RPC
 * reply, worker.go:144). A device that is not present -- DGREP_DEVICE=99 on an
 * 8-GPU node, or no GPU at all -- is DGREP_E_HIP; a DGREP_DEVICE that is not a
 * non-negative integer is DGREP_E_INVALID. */
int dgrep_pick_device(int worker_id, int* device);
int dgrep_open(int device, dgrep_ctx** ctx);
void dgrep_close(dgrep_ctx* ctx);
const char* dgrep_last_error(dgrep_ctx* ctx);
/* Use an existing hipStream_t (e.g. torch.cuda.current_stream().cuda_stream);
 * NULL selects the context's own stream. */
int dgrep_set_stream(dgrep_ctx* ctx, void* hip_stream);
/* Loads a compiled pattern: builds its images on the host
 * (csrc/runtime/pattern_image.h, build_pattern_image: the stepper choice and
 * every table; constants in csrc/kernels/pattern_layout.h and
 * scan_common.h), uploads them into fresh device allocations, then commits.
 * Failure rule: a refusal found on the host -- DGREP_E_INVALID (malformed
 * blob), DGREP_E_UNSUPPORTED (the stepper dgrep_set_stepper forces cannot run
 * this DFA) -- leaves the context exactly as it was: a previously loaded
 * pattern stays loaded and usable, and streams and jobs opened under it stay
 * valid. A HIP failure during the upload (DGREP_E_HIP) frees what the call
 * allocated and leaves the previous pattern as well. Only a successful load
 * replaces the pattern and invalidates the streams and jobs opened before. */
int dgrep_load_dfa(dgrep_ctx* ctx, const void* blob, size_t n);
/* Stepper selection for later dgrep_load_dfa calls (tests / tuning only; the
 * default picks by size: <= 8 states Sheng; else the pair stepper if its
 * two-byte table fits in LDS; else <= 256 states the u8 table; else the
 * filter: the DFA's shallowest states in LDS, lines that leave them verified
 * on the whole DFA).
 * force: 0 = that default, 2 = the u8 table (<= 256 states), 3 = pair
 * (dgrep_load_dfa fails with DGREP_E_UNSUPPORTED if it does not fit), 4 =
 * filter (the default above 256 states). 1 and 5 (the wide and word steppers
 * of earlier rounds, measured slower and removed) and anything outside 0-5 are
 * DGREP_E_INVALID. filter_rows != 0 caps the filter's LDS-resident rows (its
 * cut then sends nearly every line to verification). */
int dgrep_set_stepper(dgrep_ctx* ctx, int force, uint32_t filter_rows);
/* Tests / tuning: lane chunk of the Sheng (<= 8-state), pair and filter
 * steppers for later scans. 0 (default) = adaptive: the compiled chunk (4 KiB;
 * pair 4.5 KiB), doubled while every resident wave still gets a tile and the
 * matching lines the previous scan's density predicts fill at most a quarter
 * of a lane's record capacity, up to 32 KiB (Sheng), 64 KiB (filter) or 9 KiB (pair). Otherwise a
 * multiple of 128 in [4096, 65536] (the LDS slots hold 16-bit chunk offsets;
 * a line starting exactly at a 64 KiB chunk end is flagged separately);
 * anything else is DGREP_E_INVALID and leaves the setting unchanged. No effect
 * on the u8 table stepper (fixed 2 KiB chunks). */
int dgrep_set_lane_chunk(dgrep_ctx* ctx, uint32_t chunk_bytes);

/* Host bytes -> H2D -> scan -> D2H results. This is the call Map makes.
 * The H2D leg is the worker's split ingest (the bytes map_reduce/worker.go:72-76
 * reads with os.ReadFile and passes to Map at worker.go:141): pieces are
 * copied by CPU threads into pinned staging buffers while the copy engine
 * DMAs the previous piece (dgrep_set_ingest). */
int dgrep_scan(dgrep_ctx* ctx, const uint8_t* data, size_t n, dgrep_result* out);
/* Ingest pipeline of dgrep_scan: chunk_bytes per pinned staging buffer
 * (0 = one pageable hipMemcpyAsync, no staging), nbufs buffers in rotation,
 * threads CPU threads per piece copy (0 keeps the current value). Defaults:
 * 64 MiB x 4 buffers x 4 threads. */
int dgrep_set_ingest(dgrep_ctx* ctx, size_t chunk_bytes, int nbufs, int threads);
/* Wall time (ms) of the last dgrep_scan's ingest (host -> HBM), 0 for the
 * direct path. */
int dgrep_last_ingest_ms(dgrep_ctx* ctx, float* ms);
void dgrep_result_free(dgrep_result* r);

/* ---- partition + intermediate writer (map_reduce/worker.go:13-17,78-109) ---
 * The worker's writeMapOutput over one split's Map output, on the GPU: each
 * matching line's KeyValue{Key: Sprintf("%s (line number #%v)", filename,
 * line_no), Value: line} (application/grep.go:25-28) goes to partition
 * ihash(Key) % nreduce (FNV-1a 32 & 0x7fffffff, worker.go:13-17) as the line
 * json.NewEncoder(f).Encode(&kv) writes ({"Key":...,"Value":...}\n, HTML
 * escaping on, invalid UTF-8 as \ufffd, worker.go:92-93), in Map output
 * (line) order inside each partition. Partition p's bytes are
 * bytes[begin[p]:end[p]] -- exactly the content of mr-<task>-<p>. */
typedef struct {
  uint32_t nreduce;
  uint64_t total;   /* bytes over all partitions */
  uint64_t* begin;  /* nreduce byte offsets into bytes */
  uint64_t* end;
  uint8_t* bytes;
} dgrep_partitions;

/* Host split -> ingest -> scan -> encode -> host partitions (the Map +
 * writeMapOutput of one map task). A value that needs escaping and has at
 * least `long value` bytes (dgrep_set_long_value) is escaped by many workgroups
 * at once; dgrep_last_encode_stats says how many values took that path. */
int dgrep_map_partitions(dgrep_ctx* ctx, const uint8_t* data, size_t n, const char* filename, size_t fn,
                         uint32_t nreduce, dgrep_partitions* out);
void dgrep_partitions_free(dgrep_partitions* p);
/* Device form over dgrep_scan_device's records: writes into d_out (out_cap
 * bytes; *total receives the bytes needed -- if larger, call again with a
 * bigger buffer); part_begin/part_end are host arrays of nreduce entries.
 * d_data need not be aligned; the long-value path reads no byte outside
 * d_data[0, n) and writes no byte of a line that does not fit below out_cap.
 * Its tables are sized for values that lie apart, as a scan's do: where records
 * made by hand overlap so that their chunks outnumber them, the values that do
 * not fit are escaped by one lane each (same bytes, at 2.6 MB/s a value). */
int dgrep_encode_device(dgrep_ctx* ctx, const void* d_data, size_t n, const uint64_t* d_line_no,
                        const uint64_t* d_start, const uint64_t* d_len, uint64_t count, const char* filename,
                        size_t fn, uint32_t nreduce, void* d_out, uint64_t out_cap, uint64_t* part_begin,
                        uint64_t* part_end, uint64_t* total);
/* Device time (ms) of the last encode (HIP events on the context stream). */
int dgrep_last_encode_ms(dgrep_ctx* ctx, float* ms);
/* What the last encode of dgrep_map_partitions, dgrep_encode_device,
 * dgrep_map_partitions_batch, dgrep_encode_batch_device or dgrep_grep_job did.
 * Where a call retries with a larger buffer, the last attempt, not the sum.
 * After dgrep_job_finish: the sums over the job's packs. An encode of the
 * window route (partition streams, a job's windows) does not touch it. */
typedef struct {
  uint64_t records;      /* records of the last resident or batch encode */
  uint64_t long_values;  /* values the chunked (many-workgroup) path took */
  uint64_t long_chunks;  /* their chunks */
  float encode_ms;       /* = dgrep_last_encode_ms */
} dgrep_encode_stats;
/* Sized getter, as dgrep_last_scan_stats: writes min(out_size, its own size)
 * bytes, a larger caller struct gets its tail zeroed, out_size 0 is
 * DGREP_E_INVALID; fields are only ever appended. */
int dgrep_last_encode_stats(dgrep_ctx* ctx, dgrep_encode_stats* out, size_t out_size);

/* ---- reduce task (map_reduce/worker.go:22-68,161-165; grep.go:38-40) ------
 * One reduce task of the grep job on the GPU: `data` = the concatenated
 * mr-<map>-<r> files of partition r (json.Encoder KeyValue lines, as
 * readReduceInput decodes them); the result is one "key value\n" line
 * (fmt "%v %v\n" of the raw strings) per distinct key with one of its values
 * (the grep Reduce returns values[0] after an unstable sort, so any value of
 * a duplicated key is a valid result): here the value of the key's FIRST
 * line, in input order of the kept lines (the reference writes them in Go map
 * order, i.e. unordered). Accepted is the compact two-field form
 * {"Key":"<json string>","Value":"<json string>"}\n byte for byte, with any
 * JSON string encoding/json's decoder accepts -- not only json.Encoder's
 * canonical spelling: \/ and \uXXXX in either hex case, escaped or raw runes,
 * and raw invalid UTF-8, each byte of which becomes U+FFFD as in the decoder.
 * Keys are compared decoded, so two spellings of one key are one key. Every
 * other line -- whitespace, other field order or names, a third field, a last
 * line without '\n', even where the decoder would take it -- fails the call
 * with DGREP_E_INVALID (never guessed); dgrep_last_error names the first such
 * line. */
typedef struct {
  uint64_t lines_in; /* KeyValue lines read */
  uint64_t total;    /* output bytes */
  uint8_t* bytes;    /* the content of mr-out-<r> */
} dgrep_reduce_out;
int dgrep_reduce(dgrep_ctx* ctx, const uint8_t* data, size_t n, dgrep_reduce_out* out);
void dgrep_reduce_free(dgrep_reduce_out* r);

/* HBM-resident split (the data never leaves the device): results are written
 * to caller-provided device arrays of `capacity` entries; *count receives
 * the number of matching lines (if > capacity, nothing beyond capacity is
 * written: call again with a larger capacity). Asynchronous on the context
 * stream except for the 8-byte count readback.
 *
 * The capacity contract, on every stepper and pass:
 * - *count is exact whatever the capacity (0 is a size query), and so is
 *   dgrep_last_scan_stats' `matches`.
 * - Entries at index >= capacity are never written.
 * - *count <= capacity (a full call): entries [0, *count) are the records;
 *   entries [*count, capacity) are not written.
 * - *count > capacity (a short call): entries [0, capacity) are unspecified --
 *   some paths order the first `capacity` records, others write nothing. Call
 *   again; a short call leaves nothing behind that changes a later call's
 *   result.
 * d_data must be 16-byte aligned when n > 0, else DGREP_E_INVALID with nothing
 * written (a MATCH_NONE pattern returns before the check). With n == 0
 * d_data is not read and may be unaligned or NULL: the split is the one empty
 * line, and if the pattern matches it *count = 1 and, given capacity >= 1, the
 * record is (1, 0, 0). A DGREP_DFA_MATCH_NONE pattern gives *count = 0 and
 * touches nothing. */
int dgrep_scan_device(dgrep_ctx* ctx, const void* d_data, size_t n, uint64_t* d_line_no, uint64_t* d_start,
                      uint64_t* d_len, uint64_t capacity, uint64_t* count);

/* ---- many splits in one scan ------------------------------------------------
 * The reference job is one map task per input file (map_reduce/coordinator.go:
 * 312,329-333), so a worker usually holds many small splits, and a split far
 * below the GPU's capacity leaves most of it idle. The batch form scans k
 * splits in one launch: they are packed as P = s_0 '\n' s_1 '\n' ... '\n'
 * s_{k-1} (one '\n' between consecutive splits, none after the last), whose
 * strings.Split(P, "\n") is exactly the concatenation of the splits' own line
 * lists (an empty split is one empty line; a split ending in '\n' keeps its
 * empty last line), and each line is matched as its own string as before. One
 * scan of P therefore finds every split's matching lines in order; the GPU then
 * rebases line numbers and starts per split.
 *
 * Records are in split order, then line order; split s owns records
 * [split_begin[s], split_begin[s+1]) (empty for a split with no match). */
typedef struct {
  uint64_t count;        /* matching lines over all splits */
  uint64_t* line_no;     /* 1-based within its split */
  uint64_t* start;       /* byte offset within its split */
  uint64_t* len;
  uint32_t* split;       /* index into the caller's arrays */
  uint64_t nsplits;
  uint64_t* split_begin; /* nsplits+1: split s owns records [split_begin[s], split_begin[s+1]) */
} dgrep_batch_result;

/* Host splits data[i][0 : n[i]) -> packed while ingested (the same staging
 * ring and dgrep_set_ingest settings as dgrep_scan; the packed buffer is never
 * built on the host above the 4 MiB direct path) -> one scan -> host results.
 * DGREP_E_INVALID, with *out zeroed and before any GPU call: a null ctx, out,
 * data or n; nsplits == 0 or > UINT32_MAX; a null data[i] with n[i] != 0; split
 * lengths whose sum overflows. No DFA loaded: DGREP_E_NO_DFA. A
 * DGREP_DFA_MATCH_NONE pattern gives count 0 and an all-zero split_begin.
 * dgrep_last_scan_stats afterwards describes the scan of the packed buffer
 * (matches = the total); dgrep_last_kernel_ms stays scan plus overflow pass. */
int dgrep_scan_batch(dgrep_ctx* ctx, const uint8_t* const* data, const size_t* n, size_t nsplits,
                     dgrep_batch_result* out);
void dgrep_batch_result_free(dgrep_batch_result* r);

/* Device form: the caller packed P itself (n_packed = sum of split_len +
 * nsplits - 1 bytes at d_packed, 16-byte aligned like dgrep_scan_device's
 * split -- DGREP_E_INVALID with nothing written otherwise, unless n_packed == 0,
 * when d_packed is not read and may be unaligned or NULL; the other pointers
 * need no alignment beyond their type's). Follows
 * dgrep_scan_device's contract: `capacity` entries per result array, *count =
 * the number of matching lines; if *count > capacity nothing is written beyond
 * capacity, d_split_begin is not valid and the caller calls again. d_split_begin
 * (nsplits + 1 device entries) may be NULL. DGREP_E_INVALID before any GPU
 * call: the checks of dgrep_scan_batch, and split lengths that do not add up
 * to n_packed. A byte other than '\n' where a separator belongs is
 * DGREP_E_INVALID too (the message names the split) with *count = 0. Adds one
 * host synchronisation to the scan's own. */
int dgrep_scan_batch_device(dgrep_ctx* ctx, const void* d_packed, size_t n_packed,
                            const uint64_t* split_len /* host, nsplits */, size_t nsplits,
                            uint64_t* d_line_no, uint64_t* d_start, uint64_t* d_len, uint32_t* d_split,
                            uint64_t* d_split_begin /* nsplits+1 device entries, may be NULL */,
                            uint64_t capacity, uint64_t* count);

/* Device time (ms, HIP events) of the last batch call's own kernels: counting
 * the lines before every split (one more read of the packed buffer) and the
 * per-split ranges + rebase of the records. */
int dgrep_last_batch_ms(dgrep_ctx* ctx, float* newline_ms, float* rebase_ms);

/* ---- a split consumed in windows: any size in a fixed device footprint -------
 * The reference makes one map task per input file, so a split is one unbounded
 * string (map_reduce/worker.go:72-76), and dgrep_scan keeps all of it in HBM.
 * The windowed forms consume the split in windows of window_bytes: the device
 * holds two window buffers, and while one is scanned the next piece is DMA'd
 * into the other. A window's bytes up to its last '\n' are exactly the lines
 * it completed (strings.Split of that region, the '\n' excluded); what follows
 * the '\n' is the unfinished line and is carried to the front of the other
 * buffer. Records are rebased by the running byte and line counts, so the
 * result is bit for bit dgrep_scan's on the concatenated bytes, however the
 * stream is cut. A window without a '\n' completes no line and the buffers
 * grow by it: the device footprint is bounded by the window plus the longest
 * unfinished line, not by the split.
 *
 * DGREP_STREAM_BOUNDED / dgrep_scan_bounded make the bound unconditional. The
 * DFA restarts only at '\n' and a line matches iff the state at its end steps
 * to start_m on '\n' (dgrep_blob.h), so an unfinished line needs only its
 * state kept. Once a full window of bytes holds no '\n' they are folded: a
 * device pass walks them from the carried state (from start at the line's
 * first fold) to the exit state, in parallel and exactly for any DFA, and the
 * bytes are forgotten. Less than one window is ever carried as bytes, so each
 * of the two buffers holds fewer than 2 * window_bytes (plus 320 of padding),
 * whatever the input. When the line's '\n' arrives, its last bytes are walked
 * from the carried state and the verdict yields the line's one record -- its
 * start and length reach back over the folded bytes -- in place of what the
 * window's scan made of those last bytes alone. The records stay bit for bit
 * dgrep_scan's. A fold adds no host synchronisation. A folded line's bytes are
 * gone, so a bounded stream returns no values: a worker re-reads them from
 * start and len. A DGREP_DFA_PARTIAL pattern has no exact state past CAND and
 * is refused.
 *
 * window_bytes: a multiple of 4096 in [4096, 2^40], else DGREP_E_INVALID.
 * Ingest goes through dgrep_scan's staging ring and the dgrep_set_ingest
 * settings; a window below 4 MiB takes one pageable copy.
 * Afterwards dgrep_last_scan_stats reports, over the call's windows, the sums
 * of matches, tiles, overflow_lanes, candidates, pending, scan_attempts, the
 * long-line tallies (the 32-bit ones saturate) and the three ms fields;
 * stepper, lane_chunk and lane_slots are the last non-empty window's.
 * dgrep_last_kernel_ms is the sum over the windows. */

/* dgrep_scan with the split never resident as a whole: bit for bit dgrep_scan's
 * result. The one-shot over dgrep_stream_open, _feed(data, n), _finish without
 * values; the context holds no stream when it returns. Argument checks as
 * dgrep_scan's (result zeroed), plus window_bytes. */
int dgrep_scan_windowed(dgrep_ctx* ctx, const uint8_t* data, size_t n, size_t window_bytes, dgrep_result* out);

/* dgrep_scan_windowed with lines longer than the window folded into their DFA
 * state: open(DGREP_STREAM_BOUNDED), feed, finish. The same argument checks and
 * the same result, bit for bit dgrep_scan's. A DGREP_DFA_PARTIAL pattern:
 * DGREP_E_UNSUPPORTED with a message. */
int dgrep_scan_bounded(dgrep_ctx* ctx, const uint8_t* data, size_t n, size_t window_bytes, dgrep_result* out);

/* The streaming form, for a caller that never holds the whole split: feed the
 * pieces as they are read, take each call's completed matching lines. A stream
 * belongs to its context (one call at a time per context, as everywhere) and is
 * closed before it. */
typedef struct dgrep_stream dgrep_stream;
enum {
  DGREP_STREAM_VALUES = 1u << 0, /* also return the matching lines' bytes */
  DGREP_STREAM_BOUNDED = 1u << 1 /* fold a line that outgrows the window into its DFA state (see above) */
};
typedef struct {
  uint64_t count;      /* lines COMPLETED by this call that match */
  uint64_t* line_no;   /* 1-based in the whole stream */
  uint64_t* start;     /* byte offset in the whole stream */
  uint64_t* len;
  uint64_t* value_off; /* count + 1, only with DGREP_STREAM_VALUES, else NULL */
  uint8_t* values;     /* line r = values[value_off[r] : value_off[r+1]) */
} dgrep_stream_result;
/* DGREP_E_INVALID before any GPU call: a null ctx or stream pointer, unknown
 * flag bits, a bad window_bytes. No DFA loaded: DGREP_E_NO_DFA.
 * DGREP_STREAM_BOUNDED: with DGREP_STREAM_VALUES it is DGREP_E_INVALID (a
 * folded line's bytes are gone); it is a property of the loaded pattern, so
 * without one it is DGREP_E_INVALID as well, and with a DGREP_DFA_PARTIAL
 * pattern DGREP_E_UNSUPPORTED -- each with a message and no stream. */
int dgrep_stream_open(dgrep_ctx* ctx, size_t window_bytes, uint32_t flags, dgrep_stream** stream);
/* A feed may have any length: n == 0 does nothing, a feed longer than the
 * window is cut internally, and one result holds every line the feed completed
 * (the line a feed's last '\n' ends included; the bytes after it wait for the
 * next call). `data` is borrowed for the call only. DGREP_E_INVALID, result
 * zeroed, before any GPU call: a null stream or out, n without data, a feed
 * after dgrep_stream_finish, and a dgrep_load_dfa on the context since the
 * stream was opened (with a message). A DGREP_DFA_MATCH_NONE pattern returns
 * count 0 and copies nothing. A HIP error or out-of-memory mid-stream leaves
 * the stream unusable: every later call returns the same status;
 * dgrep_stream_close stays safe. */
int dgrep_stream_feed(dgrep_stream* stream, const uint8_t* data, size_t n, dgrep_stream_result* out);
/* The stream's last line: its record if it matches, else nothing. That line
 * may be the empty one after a final '\n', or the one empty line of an empty
 * stream. */
int dgrep_stream_finish(dgrep_stream* stream, dgrep_stream_result* out);
void dgrep_stream_result_free(dgrep_stream_result* r);
void dgrep_stream_close(dgrep_stream* stream);
/* windows scanned, device bytes of the two window buffers now, longest carried
 * tail, cut-pass ms (HIP events) -- over the stream's life; any pointer may be
 * NULL. The carried tail is measured to the end of its line: max_carry is the
 * length of the longest line that lay across a window boundary (or of the
 * unfinished tail, while that is longer). */
int dgrep_stream_stats(dgrep_stream* stream, uint64_t* windows, uint64_t* data_bytes, uint64_t* max_carry,
                       float* cut_ms);
/* A bounded stream's folds over its life (all 0 on any other stream): windows
 * folded, their bytes, chunks walked (folds, line ends and the finish), chunks
 * whose guesses missed the true entry state and were walked again, and the
 * walks' device time (ms, HIP events). Any pointer may be NULL. With a bounded
 * stream max_carry above is still the true length of the longest line across a
 * window boundary, folded bytes included. Asking for guess_misses or walk_ms
 * waits for the stream's queued work. */
int dgrep_stream_carry_stats(dgrep_stream* stream, uint64_t* folds, uint64_t* folded_bytes, uint64_t* chunks,
                             uint64_t* guess_misses, float* walk_ms);

/* ---- whole map tasks over a batch: every split's intermediate files ---------
 * A map task ends at its files mr-<task>-<p>, one per reduce partition
 * (map_reduce/worker.go:78-109). The batch form of dgrep_map_partitions writes
 * them for k splits with k filenames from one scan and one encode. Cell (s, p)
 * holds the bytes of mr-<s>-<p>, exactly what dgrep_map_partitions(split s,
 * filename s, nreduce) returns for partition p: Key = Sprintf("%s (line number
 * #%v)", filename[s], line_no) with line_no counted within split s, partition
 * = ihash(Key) % nreduce, lines in line order. Cells are contiguous,
 * split-major, then partition: cell c = s * nreduce + p occupies
 * bytes[cell_off[c] : cell_off[c+1]); cell_off has nsplits * nreduce + 1
 * entries, cell_off[0] = 0, the last one = total; an empty cell has equal
 * offsets. Filenames may have any length. */
typedef struct {
  uint64_t nsplits;
  uint32_t nreduce;
  uint64_t total;     /* bytes over all cells */
  uint64_t* cell_off; /* nsplits * nreduce + 1 */
  uint8_t* bytes;
} dgrep_batch_partitions;

/* Host splits and filenames (filename[i][0 : fn[i]), raw bytes) -> packed
 * ingest -> batch scan -> batch encode -> host bytes. DGREP_E_INVALID, with *out
 * zeroed and before any GPU call: the checks of dgrep_scan_batch; a null
 * filename or fn array; a null filename[i] with fn[i] != 0; nreduce outside
 * 1..65535. DGREP_E_UNSUPPORTED (with a message): nsplits * nreduce >= 2^32, or
 * 2^32 or more matching lines. No DFA loaded: DGREP_E_NO_DFA. A
 * DGREP_DFA_MATCH_NONE pattern gives total 0 and an all-zero cell_off. */
int dgrep_map_partitions_batch(dgrep_ctx* ctx, const uint8_t* const* data, const size_t* n,
                               const char* const* filename, const size_t* fn, size_t nsplits, uint32_t nreduce,
                               dgrep_batch_partitions* out);
void dgrep_batch_partitions_free(dgrep_batch_partitions* p);

/* ---- the windowed map task: a streamed split's intermediate files -------------
 * A partition stream is a windowed stream (above) that returns encoded
 * partition pieces instead of records: the worker that streams its file gets
 * the bytes to append to mr-<task>-<p>, with the key formatting, ihash, JSON
 * escaping and partitioning done on the device, window by window. It has its
 * own open call (no flag bit of dgrep_stream_open) and no bounded form: a
 * folded line's bytes are gone, and its value could not be written.
 *
 * Result: dgrep_batch_partitions with ROWS in place of splits, freed with
 * dgrep_batch_partitions_free. A row is one window of the call that completed
 * at least one matching line, in stream order; nsplits is the number of rows;
 * cell c = row * nreduce + p holds the bytes that window adds to
 * mr-<task>-<p>. cell_off has nsplits * nreduce + 1 entries; with no row it is
 * the single entry 0, total is 0 and bytes is NULL.
 *
 * Contract: fix a partition p, take all feeds in order and then the finish, and
 * concatenate cells (0,p), (1,p), ... of each result: that is bit for bit
 * partition p of dgrep_map_partitions(whole split, filename, nreduce), however
 * the stream is cut into feeds and whatever the window. The line numbers in the
 * keys are the stream's own.
 *
 * The layout needs no merge and feeds the reduce directly: it is
 * dgrep_reduce_batch_device's segment convention (segment g belongs to
 * partition g % nparts), so the cells of a big file are batch-reduce input
 * with seg_off = cell_off and nparts = nreduce.
 *
 * Footprint: the two window buffers, the encoder's per-record scratch, and ONE
 * window's encoded bytes (dgrep_stream_partition_stats, enc_device_bytes). A
 * partition stream keeps no record arrays. dgrep_last_scan_stats and
 * dgrep_last_kernel_ms behave as for any windowed call; dgrep_last_encode_ms
 * is the sum over the call's windows.
 *
 * A value that needs escaping and has at least `long value` bytes
 * (dgrep_set_long_value) is escaped by many workgroups at once, as in
 * dgrep_map_partitions: minified JSON, binaries and logs with embedded blobs
 * cost what their bytes cost.
 *
 * DGREP_E_INVALID before any GPU call, result zeroed: the checks of
 * dgrep_stream_open / dgrep_stream_feed; filename == NULL with fn != 0; nreduce
 * outside 1..65535. DGREP_E_INVALID with a message naming the mismatch:
 * dgrep_stream_feed / dgrep_stream_finish on a partition stream, the
 * _partitions calls on a record stream. No DFA loaded: DGREP_E_NO_DFA. A
 * DGREP_DFA_MATCH_NONE pattern gives empty results and copies nothing.
 * DGREP_E_UNSUPPORTED (with a message): 2^32 or more matching lines in one
 * window. A load on the context mid-stream, a feed after finish and a sticky
 * HIP error behave as in record streams. DGREP_DFA_PARTIAL patterns work. */
int dgrep_stream_open_partitions(dgrep_ctx* ctx, size_t window_bytes, const char* filename, size_t fn,
                                 uint32_t nreduce, dgrep_stream** stream);
int dgrep_stream_feed_partitions(dgrep_stream* stream, const uint8_t* data, size_t n, dgrep_batch_partitions* out);
int dgrep_stream_finish_partitions(dgrep_stream* stream, dgrep_batch_partitions* out);
/* open, feed(data, n), finish, both results joined into one (the finish
 * contributes at most one more row); the context holds no stream afterwards. */
int dgrep_map_partitions_windowed(dgrep_ctx* ctx, const uint8_t* data, size_t n, size_t window_bytes,
                                  const char* filename, size_t fn, uint32_t nreduce, dgrep_batch_partitions* out);
/* Over the stream's life: rows returned, their bytes, values the long-value
 * path took, the device buffer of encoded bytes now (one window's), the
 * encoder's device ms (HIP events). All 0 on a record stream. Any pointer may
 * be NULL. */
int dgrep_stream_partition_stats(dgrep_stream* stream, uint64_t* rows, uint64_t* out_bytes, uint64_t* long_values,
                                 uint64_t* enc_device_bytes, float* encode_ms);
/* Tests / tuning, like dgrep_set_lane_chunk: the value length at and above
 * which an escaped value takes the partition writers' parallel path. 0 = the
 * built-in default (256 in the window writer, 768 in the resident and the
 * batch writer); else a multiple of 64 in [256, 2^30]; anything else is
 * DGREP_E_INVALID and leaves the setting unchanged. Governs all three writers
 * (resident, batch, window) and what is built on them; 2^30 forces the
 * one-lane path everywhere. */
int dgrep_set_long_value(dgrep_ctx* ctx, uint32_t bytes);

/* Device form: the records exactly as dgrep_scan_batch_device returned them
 * over the same packed buffer (line_no and start relative to the record's
 * split, d_split filled; `count` of them) -> every cell's lines in d_out
 * (4-byte aligned). Follows dgrep_encode_device's capacity contract: *total =
 * the bytes needed, nothing is written at or past out_cap; if *total > out_cap
 * cell_off (host, nsplits * nreduce + 1 entries) is still valid and the caller
 * calls again with a larger buffer. Records from anywhere else -- a start or
 * len outside its split, a split id >= nsplits, another order -- are the
 * caller's responsibility, as with dgrep_encode_device: they are not checked.
 * DGREP_E_INVALID before any GPU call, with *total = 0: the checks of
 * dgrep_scan_batch_device (null ctx / total / cell_off / split_len, nsplits,
 * d_packed, split lengths that do not add up to n_packed), `count` without the
 * four record arrays, out_cap without d_out, and the filename and nreduce
 * checks above. DGREP_E_UNSUPPORTED: nsplits * nreduce >= 2^32 or count >=
 * 2^32. dgrep_last_encode_ms reports the encode's device time. Long escaped
 * values take the parallel path as in dgrep_encode_device: no byte outside
 * d_packed[0, n_packed) is read. */
int dgrep_encode_batch_device(dgrep_ctx* ctx, const void* d_packed, size_t n_packed,
                              const uint64_t* split_len /* host, nsplits */, size_t nsplits,
                              const uint64_t* d_line_no, const uint64_t* d_start, const uint64_t* d_len,
                              const uint32_t* d_split, uint64_t count, const char* const* filename, const size_t* fn,
                              uint32_t nreduce, void* d_out, uint64_t out_cap,
                              uint64_t* cell_off /* host, nsplits*nreduce+1 */, uint64_t* total);

/* ---- every reduce task of a job in one pass; the whole job in one call ------
 * A job ends at its files mr-out-<r> (map_reduce/worker.go:22-68,161-165, with
 * the grep plugin's Reduce = values[0], application/grep.go:38-40). The batch
 * form of dgrep_reduce runs all reduce tasks from one buffer in one launch
 * train. The buffer is cut into segments by seg_off[nseg + 1] (ascending,
 * seg_off[0] = 0, the last entry = n; no separator byte between segments);
 * segment g belongs to partition g % nparts, and partition p's reduce input
 * is its segments in ascending g, concatenated -- the mr-*-<p> files
 * readReduceInput reads one after the other. So R separate inputs are nseg =
 * nparts = R, and the batch writer's cells as they are: nseg = nsplits *
 * nreduce, nparts = nreduce, seg_off = cell_off. For each partition the result
 * is exactly the bytes dgrep_reduce returns for that partition's concatenated
 * input (the same accepted line language, the first line of every distinct
 * decoded key, in input order); the same key in two partitions is two keys.
 * Partitions lie in order in `bytes`: mr-out-<p> = bytes[part_off[p] :
 * part_off[p+1]), part_off[0] = 0, the last entry = total, an empty partition
 * has equal offsets. Every non-empty segment must end in '\n' (the end of a
 * file of whole lines): one that does not is malformed input even where its
 * last line, fused with the next segment's first, would parse. Malformed input
 * fails the whole call with DGREP_E_INVALID and nothing is returned;
 * dgrep_last_error names the first malformed line as partition p (0-based)
 * and line (1-based, within that partition's input) -- the lowest partition,
 * then the lowest line; a segment without its final '\n' counts as its last
 * line. */
typedef struct {
  uint32_t nparts;
  uint64_t total;     /* bytes over all partitions */
  uint64_t* part_off; /* nparts + 1: mr-out-<p> = bytes[part_off[p] : part_off[p+1]) */
  uint64_t* lines_in; /* nparts: KeyValue lines read for partition p */
  uint8_t* bytes;
} dgrep_reduce_batch_out;

/* R = nparts reduce tasks: data[p][0 : n[p]) = the concatenated mr-*-<p> files.
 * The inputs are ingested back to back through the staging ring and the
 * dgrep_set_ingest settings (never concatenated on the host above the 4 MiB
 * direct path). Needs no DFA. DGREP_E_INVALID, with *out zeroed and before any
 * GPU call: a null ctx, out, data or n; nparts 0 or above 65535; a null
 * data[p] with n[p] != 0; lengths whose sum overflows. All inputs empty:
 * DGREP_OK with total 0 and all-zero part_off and lines_in (no GPU call).
 * DGREP_E_UNSUPPORTED (with a message): 2^32 or more lines. */
int dgrep_reduce_batch(dgrep_ctx* ctx, const uint8_t* const* data, const size_t* n, size_t nparts,
                       dgrep_reduce_batch_out* out);
void dgrep_reduce_batch_free(dgrep_reduce_batch_out* r);

/* Device form: d_data[0 : n) (16-byte aligned when n > 0) and its segment
 * table -> every partition's bytes in d_out (4-byte aligned). Follows
 * dgrep_encode_batch_device's capacity contract: *total = the bytes needed,
 * nothing is written at or past out_cap; part_off (host, nparts + 1) and
 * lines_in (host, nparts, may be NULL) are valid whenever the input is well
 * formed, even when *total > out_cap -- the caller then calls again with a
 * larger buffer. DGREP_E_INVALID before any GPU call, with *total = 0: a null
 * ctx, total, part_off or seg_off; nseg or nparts 0; nseg not a multiple of
 * nparts; seg_off[0] != 0, a descending seg_off or seg_off[nseg] != n; n
 * without d_data; out_cap without d_out; a d_data that is not 16-byte
 * aligned. DGREP_E_UNSUPPORTED with a message
 * naming the limit (checked before seg_off is read): nparts above 65535, nseg
 * >= 2^32; after counting: 2^32 or more lines. dgrep_last_reduce_ms reports the
 * pass's device time. */
int dgrep_reduce_batch_device(dgrep_ctx* ctx, const void* d_data, size_t n,
                              const uint64_t* seg_off /* host, nseg+1 */, size_t nseg, uint32_t nparts, void* d_out,
                              uint64_t out_cap, uint64_t* part_off /* host, nparts+1 */,
                              uint64_t* lines_in /* host, nparts, may be NULL */, uint64_t* total);

/* The reference's grep job on one worker's GPU, from the input splits to every
 * mr-out-<r>: packed ingest -> batch scan -> batch encode into the context's
 * device buffer -> batch reduce with seg_off = the encode's cell_off, on the
 * device -> only the outputs are copied back. The intermediate files
 * mr-<s>-<p> are a transport between workers (worker.go:78-109); within one
 * worker their bytes never leave HBM. out->nparts = nreduce; out->bytes[
 * part_off[r] : part_off[r+1]) equals dgrep_reduce over the concatenation of
 * dgrep_map_partitions_batch's cells (0, r), (1, r), ... Argument checks and
 * status codes are dgrep_map_partitions_batch's (DGREP_E_NO_DFA, the 2^32-cell
 * and 2^32-record limits included); a DGREP_DFA_MATCH_NONE pattern, or no
 * matching line, gives total 0 with all-zero part_off and lines_in.
 * Afterwards dgrep_last_scan_stats, dgrep_last_encode_ms and
 * dgrep_last_reduce_ms describe the three legs. The writer's own output
 * cannot hold a malformed line; should the reduce report one all the same, it
 * is returned as DGREP_E_INVALID with its message. This call is for a worker
 * binary that links the library: the Go plugin's Map / Reduce pair cannot
 * express a whole job. */
int dgrep_grep_job(dgrep_ctx* ctx, const uint8_t* const* data, const size_t* n, const char* const* filename,
                   const size_t* fn, size_t nsplits, uint32_t nreduce, dgrep_reduce_batch_out* out);

/* ---- the whole job in windows: files of any size to every mr-out-<r> ----------
 * dgrep_grep_job needs every input byte resident at once. A job object takes
 * the same files in the same (task) order without that: a 2 TiB log goes
 * through windows, 65,536 small files do not each pay for a window of their
 * own. Two routes, chosen per file:
 *  - pack: a file given whole (dgrep_job_add) of at most window_bytes joins the
 *    current pack, the packed buffer of dgrep_scan_batch; a pack's files plus
 *    one separator between them stay at or below window_bytes. The pack is
 *    flushed -- one packed ingest, one batch scan, one batch encode of its k
 *    files with their k filenames -- when the next file does not fit, when a
 *    file of the other route arrives, and at finish. The job keeps a copy of a
 *    packed file's bytes: `data` is borrowed for the call only. A long escaped
 *    line inside a packed file takes the parallel long-value path, as in
 *    dgrep_map_partitions_batch.
 *  - window: a file given whole with n > window_bytes, and every file given by
 *    begin / feed / end whatever its size, streams through the job's partition
 *    stream (above: the cut, the carried tail, the parallel long-value path),
 *    after the pack was flushed.
 * A flush with a matching line yields k * nreduce cells, a window that completed
 * a matching line nreduce. They never leave the device: one kernel appends the
 * bytes to a contiguous arena and the rebased cell boundaries to a device
 * segment table (segment g belongs to partition g % nreduce), and
 * dgrep_job_finish runs the batch reduce over both; only the outputs come back.
 *
 * Contract: the same files in the same order, by any mix of dgrep_job_add and
 * begin / feed / end, any cut of a file into feeds and any window_bytes, give
 * byte for byte what dgrep_grep_job(files, nreduce) returns: bytes, part_off,
 * lines_in and total. The same filename added twice yields duplicate keys and
 * the earlier file's line wins, as there.
 *
 * Device footprint: the stream's two window buffers (bounded as for a partition
 * stream of this window: the window plus the longest unfinished line); the
 * pack buffer (the context's split buffer, at most window_bytes plus 63 of
 * padding); the scan's and the encoders' per-record scratch; one window's or
 * one pack's encoded bytes; the arena -- the job's intermediate bytes,
 * proportional to the matching lines and not to the input, grown geometrically
 * with its contents kept (old and new exist together for one device copy) and
 * below twice what is used once past its first 4 KiB; the segment table (8
 * bytes per segment); at finish the reduce's scratch and output. The window
 * buffers, the encoder scratch and the encoded-bytes buffer are allocated once
 * per job; a new file resets only the stream's state.
 *
 * DGREP_E_INVALID before any GPU call (dgrep_job_finish and the one-shot with
 * *out zeroed): null pointers; a bad window_bytes (dgrep_stream_open's rule);
 * nreduce outside 1..65535; n without data; fn without filename; feed or end
 * without begin; add, begin or finish inside an open file; any call after
 * finish; a dgrep_load_dfa on the context since the job was opened (with a
 * message). No DFA loaded: DGREP_E_NO_DFA. DGREP_E_UNSUPPORTED with a message
 * naming the limit: 2^32 or more segments; 2^32 or more matching lines in the
 * job, in one pack or in one window. A HIP error, out-of-memory or a limit
 * mid-job leaves the job unusable: every later call returns the same status;
 * dgrep_job_close stays safe. A DGREP_DFA_MATCH_NONE pattern, no matching line,
 * or no file at all: DGREP_OK with total 0 and all-zero part_off and lines_in;
 * MATCH_NONE copies nothing. DGREP_DFA_PARTIAL patterns work. At finish the '\n'
 * counted in the arena must equal the records written, as in dgrep_grep_job.
 * A job belongs to its context (one call at a time per context) and is closed
 * before it. After dgrep_job_finish, dgrep_last_scan_stats, dgrep_last_kernel_ms
 * and dgrep_last_encode_ms report sums over the job's packs and windows,
 * dgrep_last_encode_stats the sums over its packs, dgrep_last_reduce_ms the
 * reduce. */
typedef struct dgrep_job dgrep_job;
int dgrep_job_open(dgrep_ctx* ctx, size_t window_bytes, uint32_t nreduce, dgrep_job** job);
/* a whole file held by the caller: any size */
int dgrep_job_add(dgrep_job* job, const uint8_t* data, size_t n, const char* filename, size_t fn);
/* a file the caller never holds: begin, feed any number of pieces, end */
int dgrep_job_file_begin(dgrep_job* job, const char* filename, size_t fn);
int dgrep_job_file_feed(dgrep_job* job, const uint8_t* data, size_t n);
int dgrep_job_file_end(dgrep_job* job);
/* every mr-out-<r>; freed with dgrep_reduce_batch_free */
int dgrep_job_finish(dgrep_job* job, dgrep_reduce_batch_out* out);
void dgrep_job_close(dgrep_job* job);
/* one-shot: open, add every file in order, finish, close */
int dgrep_grep_job_windowed(dgrep_ctx* ctx, const uint8_t* const* data, const size_t* n, const char* const* filename,
                            const size_t* fn, size_t nsplits, uint32_t nreduce, size_t window_bytes,
                            dgrep_reduce_batch_out* out);
/* What the job did so far (any time between open and close). */
typedef struct {
  uint64_t files;               /* files added, both routes */
  uint64_t packs;               /* packs flushed */
  uint64_t files_packed;        /* files that took the pack route */
  uint64_t files_windowed;      /* files that took the window route */
  uint64_t windows;             /* windows scanned (a file's finish included) */
  uint64_t rows;                /* rows of nreduce cells in the arena: a flushed file or a window with a match */
  uint64_t segments;            /* rows * nreduce */
  uint64_t arena_bytes;         /* intermediate bytes in the arena */
  uint64_t arena_device_bytes;  /* the arena's capacity now */
  uint64_t window_device_bytes; /* the two window buffers now (dgrep_stream_stats' data_bytes) */
  uint64_t long_values;         /* values the window route's parallel long-value path took */
  uint64_t arena_growths;       /* reallocations of the arena after the first */
  float scan_ms;                /* device ms, HIP events: scans (dgrep_last_kernel_ms summed) */
  float encode_ms;              /* the batch and window encoders */
  float append_ms;              /* the arena appends (the last one counts once a later call waited for it) */
  float reduce_ms;              /* the batch reduce of dgrep_job_finish */
} dgrep_job_stats;
/* Sized getter, as dgrep_last_scan_stats: writes min(out_size, its own size)
 * bytes and zeroes a larger caller struct's tail; out_size 0 is
 * DGREP_E_INVALID. Fields are only ever appended. */
int dgrep_job_stats_get(dgrep_job* job, dgrep_job_stats* out, size_t out_size);

/* Device time (ms, HIP events on the context stream) of the last batch reduce. */
int dgrep_last_reduce_ms(dgrep_ctx* ctx, float* ms);

/* ---- multi-GPU exchange -----------------------------------
 * Replaces the SFTP shipping of map output to the reducers
 * (map_reduce/coordinator.go:136-142) for workers on one node: each worker
 * process scans its split on its own GPU and the compacted match records --
 * never the line bytes -- are gathered to the reducing worker over RCCL
 * (xGMI). Callable from the Go worker through cgo like the rest of the ABI.
 * Setup: the root calls dgrep_comm_unique_id and hands the 128 bytes to the
 * other workers out of band (the worker's own channel, e.g. a file or its RPC);
 * every worker then calls dgrep_comm_open with its rank (collective: all
 * nranks must call it). The communicator uses the context's device and stream. */
#define DGREP_COMM_ID_BYTES 128
typedef struct dgrep_comm dgrep_comm;
int dgrep_comm_unique_id(void* id_out /* DGREP_COMM_ID_BYTES */);
int dgrep_comm_open(dgrep_ctx* ctx, const void* id, int nranks, int rank, dgrep_comm** comm);
void dgrep_comm_close(dgrep_comm* comm);
/* Gather every rank's records (a dgrep_scan_device result: `count` entries of
 * the three device arrays) to rank `root`, as 28-byte packed records
 * {u64 line_no, u64 start, u64 len, u32 split} (split = the caller's map task
 * id, so the root can rebuild each Key = Sprintf(filename[split], line_no),
 * application/grep.go:25), in rank order. Collective. The counts are
 * all-gathered first (8 B per rank), then one grouped send/recv moves exactly
 * sum(counts) x 28 bytes into a device buffer the communicator owns (grown as
 * needed): on the root *d_records points at it (valid until the next gather or
 * dgrep_comm_close), *total = sum(counts), and rank_counts (may be NULL)
 * receives the nranks counts. Other ranks: *d_records = NULL, *total = count. */
int dgrep_gather_records_device(dgrep_comm* comm, const uint64_t* d_line_no, const uint64_t* d_start,
                                const uint64_t* d_len, uint64_t count, uint32_t split, int root,
                                const void** d_records, uint64_t* total, uint64_t* rank_counts);
/* The same with host results on the root (SoA, malloc'd; free with
 * dgrep_gathered_free); other ranks get count 0. */
typedef struct {
  uint64_t count;
  uint64_t* line_no;
  uint64_t* start;
  uint64_t* len;
  uint32_t* split;
} dgrep_gathered;
int dgrep_gather_records(dgrep_comm* comm, const uint64_t* d_line_no, const uint64_t* d_start, const uint64_t* d_len,
                         uint64_t count, uint32_t split, int root, dgrep_gathered* out);
void dgrep_gathered_free(dgrep_gathered* g);
/* message for the communicator's last non-OK status (RCCL / HIP error text) */
const char* dgrep_comm_last_error(dgrep_comm* comm);

/* ---- bench / test tooling ------------------------------------------------ */
/* Fill d_out[0:n) with the seeded synthetic log corpus on
 * the device. kind: 0 = plain log lines, 1 = log lines with seeded
 * case-insensitive keywords planted (config 4), 2 = long lines (4 MiB mean)
 * between pages of log lines, 3 = kind 2 after one newline-free 1 GiB line,
 * 4 = kind 2 with config 4's keywords planted (csrc/kernels/synth.h). */
int dgrep_synth_corpus(dgrep_ctx* ctx, void* d_out, size_t n, uint64_t seed, int kind);
/* Host twin of dgrep_synth_corpus (same generator code): fills out[0:n). */
int dgrep_synth_corpus_host(void* out, size_t n, uint64_t seed, int kind);
/* Keyword i (0..999) of the seeded config-4 keyword set; returns its length. */
int dgrep_synth_keyword(uint64_t seed, int i, char* out16);
/* Device time (ms) of the last dgrep_scan* call's scan: the scan kernel
 * (every attempt, if the overflow list had to grow) plus the overflow pass,
 * measured with HIP events on the launch stream. */
int dgrep_last_kernel_ms(dgrep_ctx* ctx, float* ms);
/* dgrep_last_kernel_ms summed over the dgrep_scan_device calls since the
 * previous take (and their number), then reset: a benchmark reads its timed
 * steps' device time once, after them, with no host call between scans. */
int dgrep_take_kernel_ms(dgrep_ctx* ctx, double* sum_ms, uint64_t* scans);

/* What the last dgrep_scan* call did (tests, tuning, bench reports). */
typedef struct {
  uint32_t stepper;        /* 0 u8 table, 1 Sheng (<= 8 states), 3 pair (two bytes per lookup), 4 filter
                              (shallow DFA states in LDS + candidate verification) */
  uint32_t lane_chunk;     /* bytes per lane chunk */
  uint32_t lane_slots;     /* LDS slots per lane chunk for matching lines */
  uint32_t scan_attempts;  /* scan launches: one more for each buffer the scan outgrew (overflow list, pending
                              list, staging), at most 4 */
  uint64_t tiles;          /* wave tiles of the split */
  uint64_t overflow_lanes; /* lane chunks re-run by the overflow pass */
  uint64_t matches;        /* matching lines */
  float scan_ms;           /* scan kernel, all attempts */
  float overflow_ms;       /* overflow pass */
  float verify_ms;         /* filter stepper: re-run of the candidate lines on the whole DFA; Sheng: resolution
                              of the parked long lines */
  uint64_t candidates;     /* filter stepper: candidate lines dropped by that re-run */
  uint64_t pending;        /* Sheng: long lines parked by the scan and resolved from chunk maps */
  uint32_t long_guess_misses; /* filter stepper (> 256 states): segments of parked lines whose true entry state
                                 was none of the guessed ones, re-run serially from it (saturates) */
  uint32_t long_segments;     /* filter stepper: segments of parked lines entered in a non-absorbing state
                                 (saturates); both 0 when no filter line was parked */
} dgrep_scan_stats;
/* Sized getter: out_size is the caller's sizeof(dgrep_scan_stats). The library
 * writes min(out_size, its own size) bytes, so a binding built against an
 * older (shorter) layout never has bytes written past its struct; a larger
 * caller struct gets its tail zeroed. out_size 0 is DGREP_E_INVALID. The
 * layout above is the round-5 one (80 bytes); fields are only ever appended. */
int dgrep_last_scan_stats(dgrep_ctx* ctx, dgrep_scan_stats* out, size_t out_size);

/* Provenance of this library: "head=<git commit>[-dirty] arch=gfx950
 * hipflags=<tuning -D knobs>" (static string). */
const char* dgrep_build_info(void);

#ifdef __cplusplus
}
#endif
#endif
