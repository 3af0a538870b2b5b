/*
 * mpc_hip.h -- C ABI of libmpc_hip.so: the MI355X (gfx950) implementation of
 * the per-cache-line compression-size evaluator of scalable-arch/CAL_22-MPC.
 *
 * The reference has no FFI; its boundary for this path is the C++ pair
 *   comp::Compressor::CompressLine(std::vector<uint8_t>&)   src/compressor/Compressor.h:28
 *   comp::Compressor::GetResult()                           src/compressor/Compressor.h:29
 * fed by trace::Loader::GetCacheline()                      src/loader/Loader.h:77
 * from the loop compressLines()                             src/main.cpp:208-248.
 * This header is what a binding for that path would call instead: one opaque
 * evaluator per comp::VPC / comp::BDI object, a batch call that replaces the
 * per-line loop, and a flat integer statistics vector that replaces
 * VPCResult / BDIResult (src/compressor/VPC.h:36-238, BDI.h:23-88).
 *
 * Conventions: plain C types only; every function returns 0 or a negative
 * errno-style code (never throws, never exits); the caller owns all buffers;
 * one handle is used from one thread at a time.  There is NO CPU fallback:
 * without a usable HIP device the create calls fail with MPC_E_NODEVICE.
 */
#ifndef MPC_HIP_H
#define MPC_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MPC_ABI_VERSION 1

/* error codes */
#define MPC_OK            0
#define MPC_E_INVAL      -22  /* bad argument / unsupported configuration value */
#define MPC_E_NOENT       -2  /* configuration file cannot be opened */
#define MPC_E_PARSE      -74  /* configuration is not valid JSON / schema */
#define MPC_E_NODEVICE   -19  /* no HIP device / HIP runtime failure at create */
#define MPC_E_NOMEM      -12
#define MPC_E_HIP         -5  /* HIP call failed during a batch; see mpc_last_error */

typedef struct mpc_handle mpc_handle;

/* Which kernel a VPC configuration maps to (mpc_info.kernel_path). */
#define MPC_PATH_VPC_FAST     1  /* (truncated) plane- or byte-major scan, windowed tables, any root for OneBase/Diff/Weight: vpc_lane_kernel */
#define MPC_PATH_VPC_GENERIC  2  /* any table / root / scan order              */
#define MPC_PATH_BDI          3
#define MPC_PATH_FPC          4
#define MPC_PATH_BPC          5
#define MPC_PATH_SC2          6
#define MPC_PATH_PATTERN      7
#define MPC_PATH_CPACK        8  /* C-Pack with a per-line dictionary */
#define MPC_PATH_CPACK_BLOCKS 10  /* mpc_create_cpack_blocks: C-Pack with a dictionary shared by blocks of N lines, one lane per block */
#define MPC_PATH_FIT_PAIRS    11  /* mpc_create_fit_pairs: bit lengths of the byte-pair residues, one lane per pair */
#define MPC_PATH_FIT_RESIDUES 12  /* mpc_create_fit_residues: residue histogram for a base table, one lane per byte */
#define MPC_PATH_PATTERN_EVICTING 9  /* mpc_create_pattern_evicting: the analysis kernel of MPC_PATH_PATTERN, then the evicting set's passes */

typedef struct {
  int32_t abi_version;
  int32_t algorithm;        /* 0 = VPC, 1 = BDI, 2 = FPC, 3 = BPC, 4 = SC2, 5 = Pattern, 6 = C-Pack (per-line dictionary, or per block of lines: kernel_path), 7 = Fit (an analysis, pairs or residues: kernel_path) */
  int32_t line_size;        /* bytes per line (L) */
  int32_t num_modules;      /* VPC: M; BDI: 0 */
  int32_t num_clusters;     /* VPC: M+1 (cluster -1 .. M-1); BDI: 9 states; FPC: 8 prefixes; BPC: 7 patterns; SC2: 2 (warm-up, table); Pattern: 10 states; C-Pack: 6 patterns; Fit: 9 bit lengths (pairs) or 256 residues */
  int32_t hist_bins;        /* VPC: bins per cluster in the stats vector */
  int32_t kernel_path;      /* MPC_PATH_* */
  int32_t device;           /* HIP device ordinal the handle is bound to */
  uint64_t stats_len;       /* number of uint64 in the statistics vector */
} mpc_info;

/* ---- construction (replaces `new comp::VPC(configPath)`, VPC.h:244-249, and
 *      `new comp::BDI(lineSize)`, BDI.h:94-98) ------------------------------
 * device < 0 selects the current HIP device.  The VPC JSON schema is the one
 * VPC::parseConfig reads (VPC.cpp:72-330).                                  */
int mpc_create_vpc(const char *config_json_path, int device, mpc_handle **out);
int mpc_create_vpc_from_string(const char *config_json_text, int device, mpc_handle **out);
int mpc_create_bdi(unsigned line_size, int device, mpc_handle **out);   /* any multiple of 8 up to 256 (BDI.cpp:8) */
/* Limits of mpc_create_vpc*: up to 32 modules (31 prediction modules), lineSize a multiple of 4 up to
 * 256, clusters x histogram bins x 4 B <= 150 KiB (the per-workgroup histogram lives in LDS); MAE / MSE
 * reproduce the reference's running doubles bit for bit when lineSize is a power of two and to 1e-12
 * otherwise ("Deliberate deviations").
 * `new comp::FPC(lineSize)` (FPC.h:91-97): frequent pattern compression of the line's 32-bit
 * words (FPC.cpp:7-88).  Per-line output: size in bits; `selected` is written as 0.
 * One definition where the reference has undefined behaviour: a zero run ends at the end of
 * the line (FPC.cpp:26 reads past it; with that read stopped at the line end, the reference
 * gives exactly these numbers: tests/golden/ref_baseline_vectors.npz).                    */
int mpc_create_fpc(unsigned line_size, int device, mpc_handle **out);
/* `new comp::BPC(lineSize)` (BPC.h:93-99): bit-plane compression (BPC.cpp:20-185).  Per-line
 * output: size in bits (may exceed 8*L: the reference does not cap it); `selected` is 0.
 * Kept as in the source: the first word always costs 3+4 bits (`if (base = 0)`,
 * BPC.cpp:98).  Defined where the source is undefined: words are zero-extended to 64 bits
 * (BPC.cpp:42-44 copies 4 bytes into an uninitialised int64_t; the upper half is the same for
 * every word of a line and cancels in the deltas).  Pinned to the reference's own numbers by
 * tests/golden/ref_baseline_vectors.npz.                                                    */
int mpc_create_bpc(unsigned line_size, int device, mpc_handle **out);
/* `new comp::SC2(lineSize, warmupCnt)` (SC2.h:100-107): a Huffman code over the line's 32-bit little-endian words
 * (SC2.cpp:270-333), with its table built once from a warm-up sample.  Lines 0 .. S-1 of the trace (S =
 * sampling_lines; lines are counted across every call on the handle, whichever ingestion path they come through)
 * only add their words to the frequency counts and cost W x 33 bits each (W = line_size / 4, the table is still
 * empty).  When line S arrives the table is built: the 1024 most frequent words (ties: the larger word is kept),
 * the reference's own heap replayed on the host (mpc_sc2_code_lengths), code length = depth in the tree (a table of
 * one symbol has length 0).  Line S and every later line cost, per word, its code length if it is in the table and
 * 33 bits if not.  Per-line output: size in bits; `selected` is 0 for a warm-up line and 1 for a table line.
 * That build is the one blocking point of an SC2 handle: it synchronises the stream of the call that reaches line S
 * (for mpc_compress_batch_device the caller's hip_stream, which must also carry or have completed the earlier
 * warm-up calls), selects the table on the device, builds it on the host and uploads it.
 * line_size: a multiple of 4 up to 256.  sampling_lines: 1 .. with sampling_lines x line_size / 4 <= 2^28 (the
 * warm-up frequency table, two 8-byte slots per sampled word rounded up to a power of two, is allocated at creation
 * and freed after the build).  S = 0 is undefined in the reference (MPC_E_INVAL).  A new trace needs a new handle.  */
int mpc_create_sc2(unsigned line_size, uint64_t sampling_lines, int device, mpc_handle **out);
/* The reference driver's warm-up length for a trace of num_lines lines (main.cpp:110-113; numLines is the loader's
 * GetNumLines(): every row of a .npy, every complete record of a GPGPU-Sim .log): max(10000, min(num_lines / 100, 10^6)). */
uint64_t mpc_sc2_sampling_lines(uint64_t num_lines);
/* The host table builder every SC2 handle uses, without a device: code lengths of n distinct symbols with their
 * warm-up frequencies, written in input order; when n > 1024 the symbols outside the 1024 largest (freq, symbol)
 * pairs get 0xFFFF.  MPC_E_INVAL for n == 0 or a repeated symbol.                                                 */
int mpc_sc2_code_lengths(const uint32_t *symbols, const uint64_t *freqs, size_t n, uint16_t *len_out);
/* The handle's code table in ascending symbol order: *n symbols (0 before line S has been seen); symbols and lengths
 * need room for *n entries (at most 1024).                                                                          */
int mpc_sc2_table(mpc_handle *h, uint32_t *symbols, uint16_t *lengths, size_t cap, size_t *n);
/* `new comp::Pattern(lineSize)` (Pattern.h:228-252): the reference's dataset analyser.  Per line of L bytes
 * (Pattern.cpp:6-75): all bytes zero adds L to Z; all 4-byte words equal adds L to R (a zero line counts in both); an
 * equal line seen before on this handle, in this or any earlier call, adds L to T, and otherwise the line joins the
 * handle's set; the six base-delta scans B8D1 B8D2 B8D4 B4D1 B4D2 B2D1 run in that order and the first of the smallest
 * sizes below 8 L is selected; the selected scan's immediates add their B bytes each to ImplicitCounts and its other
 * values to ExplicitCounts, a line without a selection adds L to U; every byte is counted in SymbolCounts and, unless
 * the line is all-zero or all-word-same, in SymbolCountsExceptAllZerosAllWordSame.  Per-line output: the smallest size
 * + 4 bits (CompressLine's return value); `selected` is the PatternState, 0..5 or 9 (NotDefined).
 * line_size: a multiple of 8 from 8 to 256 (the reference reads past the line otherwise); checked before any device is
 * touched.  The set lives in device memory, sized at creation: (8 + line_size) x 2^25 bytes (2.25 GiB for 64-byte
 * lines) plus 64 MiB of work lists.
 * LIMIT the reference does not have: its LRU starts evicting when the 2^24-th distinct line arrives, and this handle
 * does not model eviction (mpc_create_pattern_evicting does).  A handle takes 2^24 - 1 distinct lines.  The call that brings one more fails with MPC_E_INVAL (a call
 * that does not wait for its lines, mpc_compress_batch_device, reports it at the next mpc_sync / mpc_stats_get); from
 * then on the handle refuses lines and mpc_stats_get returns the same error.  A new trace needs a new handle.        */
int mpc_create_pattern(unsigned line_size, int device, mpc_handle **out);
/* The same analyser with the reference's eviction (opt-in; mpc_create_pattern is unchanged and keeps refusing).  The
 * reference's cache is only ever asked exist() and, on a miss, put() (Pattern.cpp:109-116; LRU.h), so a hit reorders nothing
 * and it is a FIFO over insertions: a line existed before iff an equal line was inserted earlier and the stamp s of its
 * latest insertion (the number of insertions before it) satisfies s >= I - capacity, I the insertions so far: it is one
 * of the last `capacity` insertions.  A line that did not exist is inserted.  Beyond the capacity the
 * result depends on the order of the lines: a handle's calls are evaluated in the order they are made, on whichever streams.
 * capacity: 0 stands for the reference's 2^24 - 1; 1 .. 2^24 - 1 sizes the set for that capacity (small capacities
 * allocate little); anything larger is refused, like a bad line_size, before a device is touched.
 * Memory: two tables of S slots, S the smallest power of two >= 1.5 x (2 capacity + min(capacity, 2^22)), of
 * (24 + line_size) bytes per slot, plus 37 bytes per line of a launch: 2 x 2^26 x (24 + line_size) bytes at the
 * reference's capacity (4 GiB for 8-byte lines, 11 GiB for 64-byte lines).  It does not grow with the trace.
 * Statistics: the Pattern layout, [21] = insertions (every miss inserts), T = L x ([0] - [21]).  Below the capacity every
 * number equals mpc_create_pattern's.  mpc_get_info reports MPC_PATH_PATTERN_EVICTING.                              */
int mpc_create_pattern_evicting(unsigned line_size, uint64_t capacity, int device, mpc_handle **out);
/* Lines that joined the handle's set since creation: its distinct lines, or for an evicting handle its insertions (a line
 * that was evicted and comes back is inserted again).  Waits like mpc_sync; not cleared by mpc_stats_reset. */
int mpc_pattern_distinct_lines(mpc_handle *h, uint64_t *n);
/* C-Pack (reference CPACK.cpp:7-101) with a PER-LINE dictionary: what `new comp::CPACK(lineSize)` constructed afresh for
 * every line reports.  NOT the numbers of the reference's `-a CPACK` run: its driver keeps one object, so the 16-entry
 * FIFO dictionary is carried from line to line (CPACK.h:107-113, CPACK.cpp:86-93); that is sequential state, does not
 * shard, and is not offered.  A cache decompresses lines independently, and C-Pack as published starts
 * each line from a fresh dictionary: that is what is evaluated here.
 * Per line: the dictionary is a FIFO of 16 four-byte entries, all zero.  For each 4-byte word b0 b1 b2 b3 in memory
 * order: b0 = b1 = b2 = 0 is ZZZZ (2 bits) when b3 = 0 and ZZZX (12) otherwise, without a dictionary access; else the
 * first entry from the front (the oldest) with the same b0, b1 decides alone -- b2 differs MMXX (24), b3 differs MMMX
 * (16), all equal MMMM (6) -- and a hit changes nothing; without such an entry the word is XXXX (34), is pushed at the
 * back and the front entry leaves.  Per-line output: the sum of the word sizes in bits (not capped: 16 misses in a
 * 64-byte line are 544 bits); `selected` is 0.
 * dictionary_scope: MPC_CPACK_DICT_PER_LINE; MPC_CPACK_DICT_CARRIED and every other value return MPC_E_INVAL with a
 * message.  line_size: a multiple of 4 from 4 to 256.  Both are checked before any device is touched.                */
#define MPC_CPACK_DICT_CARRIED  0
#define MPC_CPACK_DICT_PER_LINE 1
int mpc_create_cpack(unsigned line_size, int dictionary_scope, int device, mpc_handle **out);
/* C-Pack with a dictionary shared by BLOCKS of block_lines lines: what one reference comp::CPACK object reports when a
 * fresh one is constructed every block_lines lines.  The handle numbers the lines it is given 0, 1, 2, ... in the order
 * of its calls, from creation or the last mpc_cpack_blocks_restart, across calls and across ingestion paths.  Block b is
 * lines [b N, (b + 1) N), N = block_lines; the last block of a trace may be short.  At the first word of line b N the
 * dictionary is 16 zero words; within the block it is carried from word to word and from line to line exactly as
 * CPACK::CompressLine does on one object (the word rules are those above).  Per-line output: that line's size in bits
 * (not capped); `selected` is 0.  Statistics: the C-Pack layout.  N = 1 gives the numbers of mpc_create_cpack.
 * What a caller must know:
 *  - The result depends on where blocks begin.  Shards of a trace must start at multiples of N (a rank's first line is
 *    line 0 of its handle), or the shards' numbers are those of another blocking.
 *  - A block is one lane's sequential work: the cost of a line grows with N, and a trace of fewer than some ten thousand
 *    blocks does not fill the device.
 *  - N beyond the length of the trace is the reference's `-a CPACK` run, one dictionary carried over all of it, evaluated
 *    by a single lane.  It is exact and slow.
 * A call, a staged chunk or a launch may end inside a block: the open block's dictionary stays in device memory and the
 * next lines continue it, whichever call, ingestion path or group brings them; the launches of one handle are chained
 * and never overlap.  mpc_stats_reset clears the statistics and leaves the open block and the position in it (as it
 * leaves SC2's line counter).
 * line_size: a multiple of 4 from 4 to 256.  block_lines: 1 .. 2^32 - 1.  Both are checked before any device is touched
 * (MPC_E_INVAL, a message that starts with "C-Pack" and names the limit).  mpc_get_info reports algorithm 6, 6 clusters
 * and MPC_PATH_CPACK_BLOCKS; mpc_kernel_form and mpc_group_form name the block length.                                  */
int mpc_create_cpack_blocks(unsigned line_size, uint64_t block_lines, int device, mpc_handle **out);
/* The next line the handle is given starts a block (and is line 0 again): for a handle that is fed a second trace.  The
 * statistics stay.  MPC_E_INVAL for every handle that mpc_create_cpack_blocks did not make.                             */
int mpc_cpack_blocks_restart(mpc_handle *h);
/* The block length the handle was created with.  MPC_E_INVAL for every other handle.                                   */
int mpc_cpack_block_lines(const mpc_handle *h, uint64_t *n);
/* Fit: the two analyses from which cal_22-mpc_amd/fit.py fits the BaseIndexTable and the DiffTable of a DiffBase module
 * to a trace (no counterpart in the reference, which ships no configuration).  bitlen8(v) = 0 for v = 0, else the position
 * of the highest set bit of v plus 1 (1..8); every residue is a uint8 difference mod 256 as in ResidueModule.cpp:34 (-1 is
 * 255 and costs 8).  Ordinary handles for every ingestion and statistics call; all counters are uint64 sums over lines,
 * so calls, shards and merged vectors add.  What an analysis does not have: a per-line result (non-NULL size_bits_out /
 * selected_out), size accounting (mpc_size_hist_enable) and a place in a group (mpc_group_create) each return MPC_E_INVAL
 * with a message that begins with "Fit".  line_size: 32, 64 or 128, checked before any device is touched.
 * Pair table: P[i][j][k], i, j in [0, L), k in [0, 9) = lines with bitlen8((line[i] - line[j]) & 255) == k.             */
int mpc_create_fit_pairs(unsigned line_size, int device, mpc_handle **out);
/* Residue histogram for a base table: V[i][v] = lines with (line[i] - line[base_table[i]]) & 255 == v.  base_table: L
 * entries, each < L (any table: forward references and base_table[i] == i included); copied.                          */
int mpc_create_fit_residues(unsigned line_size, const uint8_t *base_table, int device, mpc_handle **out);
/* The base table of an mpc_create_fit_residues handle (n >= L).  MPC_E_INVAL for every other handle.                  */
int mpc_fit_base_table(const mpc_handle *h, uint8_t *out, size_t n);
void mpc_destroy(mpc_handle *h);

int mpc_get_info(const mpc_handle *h, mpc_info *info);
/* Why a VPC configuration runs on the generic kernel (kernel_path == MPC_PATH_VPC_GENERIC, some hundred times slower
 * than the fast kernel): one sentence naming the module and the property; "" for every other handle.  The
 * `compressor` CLI prints it to stderr so that the slow path is never entered silently.                          */
const char *mpc_path_reason(const mpc_handle *h);
/* The form of the kernel the handle launches, for logs and tests: "unrolled" (a built-in instantiation of the module
 * sequence), "unrolled, general layout" (RootIndex 1..15 / whole-plane truncation), "unrolled, compiled at creation"
 * (the sequence had no built-in instantiation: hiprtc compiled it when the handle was created; "(from the cache)"
 * when a previous process had), "run-time loop", "generic".  No counterpart in the reference.                          */
const char *mpc_kernel_form(const mpc_handle *h);
/* Build check, needs no device: when the configuration's module sequence has no built-in unrolled instantiation and would
 * be compiled when a handle is created (hiprtc), compile it now for gfx950 and return the size of the
 * code object; 0 when nothing would be compiled (built in, or a layout that takes the run-time loop); negative MPC_E_*
 * with the parser's or the compiler's message in `log`.                                                             */
long long mpc_jit_compile_check(const char *config_json_text, char *log, size_t log_cap);
/* Last error text of this handle (or of the last failed create if h==NULL). */
const char *mpc_last_error(const mpc_handle *h);

/* ---- the hot path (replaces the CompressLine loop, main.cpp:237-243) -----
 * `lines` is n consecutive lines of line_size bytes in HOST memory.  They are
 * staged through pinned double buffers with hipMemcpyAsync and evaluated on
 * the device.  size_bits_out (n x uint16: CompressLine's return value) and
 * selected_out (n x int8: VPC cluster -1..M-1, or BDIState 0..8) may each be
 * NULL.  Statistics accumulate in the handle exactly as m_Stat does.  The
 * call returns when the results are in the output buffers.  Calls of up to
 * 512 lines (the per-line CompressLine of an unchanged reference driver) are
 * evaluated in place from a small pinned buffer: one launch, one stream
 * synchronisation, no staging slots.                                        */
int mpc_compress_batch(mpc_handle *h, const uint8_t *lines, uint64_t n_lines,
                       uint16_t *size_bits_out, int8_t *selected_out);

/* Same, for lines already resident in DEVICE memory (16-byte aligned) and
 * optional DEVICE output arrays; asynchronous on `hip_stream` (a hipStream_t
 * passed straight to the launch; NULL = HIP's default stream).  Statistics
 * accumulate on the device; call mpc_sync (or mpc_stats_get), which wait for the
 * whole device, before reading outputs.                                     */
int mpc_compress_batch_device(mpc_handle *h, const void *d_lines, uint64_t n_lines,
                              uint16_t *d_size_bits_out, int8_t *d_selected_out,
                              void *hip_stream);
int mpc_sync(mpc_handle *h);

/* ---- statistics (replaces VPCResult / BDIResult) -------------------------
 * Integer vector, identical on 1 GPU, N GPUs after a sum all-reduce, and the
 * CPU oracle.  VPC layout (K = M+1 clusters, index k = cluster+1,
 * B = hist_bins):
 *   [0] lines  [1] original_bits  [2] compressed_bits
 *   [3 + 6k + 0] count_k            [3 + 6k + 1] original_bits_k
 *   [3 + 6k + 2] compressed_bits_k  [3 + 6k + 3] residue_lines_k
 *   [3 + 6k + 4] sum_r_k            [3 + 6k + 5] sum_r2_k
 *   [3 + 6K + k*B + s] histogram_k[s]   (lines of cluster k with size s bits)
 * MAE_k = sum_r_k / (L * residue_lines_k), MSE_k likewise (VPC.h:62-76).
 * BDI layout: [0] lines [1] original_bits [2] compressed_bits [3..11] Counts.
 * FPC layout: [0] lines [1] original_bits (32 per word) [2] compressed_bits [3..10] Counts of
 *             Prefix0..7 (FPC.h:13-23); TotalWords = their sum.
 * BPC layout: [0] lines [1] original_bits [2] compressed_bits [3] TotalWords [4..10] Counts in
 *             BPCPattern order (BPC.h:12-21).
 * SC2 layout: [0] lines [1] original_bits [2] compressed_bits [3] warm-up lines [4] table symbols
 *             [5] words found in the table.  mpc_stats_reset clears the statistics only: the table and the
 *             handle's line counter (which line is line S) stay.
 * C-Pack layout: [0] lines [1] original_bits [2] compressed_bits [3] TotalWords (the sum of the counts) [4..9] Counts in
 *             CPACKPattern order ZZZZ ZZZX MMMM MMMX MMXX XXXX (CPACK.h:18-26), of 2 12 6 16 24 34 bits.
 * Pattern layout: [0] lines [1] 0 [2] 0 (CompResult::Update is never called: OriginalSize and CompressedSize stay 0)
 *             [3] sum of the returned sizes [4] Z [5] R [6] T [7] U [8] Total, all in bytes [9..14] ImplicitCounts
 *             [15..20] ExplicitCounts [21] lines that joined the set (an evicting handle: insertions) [22..277] SymbolCounts [278..533]
 *             SymbolCountsExceptAllZerosAllWordSame.  T = L x ([0] - [21]).  mpc_stats_reset clears the statistics,
 *             [21] included, and keeps the set: lines seen before the reset still count as seen.
 * Fit pairs layout: [0] lines [1] 0 [2] 0 (an analysis, as Pattern) [3 + (i L + j) 9 + k] P[i][j][k]; length 3 + 9 L^2.
 * Fit residues layout: [0] lines [1] 0 [2] 0 [3 + 256 i + v] V[i][v]; length 3 + 256 L.
 */
int mpc_stats_len(const mpc_handle *h, uint64_t *len);
int mpc_stats_get(mpc_handle *h, uint64_t *vec, size_t n);      /* syncs */
int mpc_stats_merge(mpc_handle *h, const uint64_t *vec, size_t n); /* += */
int mpc_stats_set(mpc_handle *h, const uint64_t *vec, size_t n);   /* = (after an all-reduce) */

/* Device-side exchange (multi-GPU without a host round trip).  The handle's device
 * accumulators ("raw" statistics: VPC [sum_r(K)] [sum_r2(K)] [histogram(K x B)], BDI
 * [Counts(9)] [compressed_bits], FPC [Counts(8)] [compressed_bits], BPC [Counts(7)] [TotalWords] [compressed_bits], SC2
 * [compressed_bits] [words_in_table], Pattern: the 531 sums of csrc/mpc_pattern.h, C-Pack [Counts(6)] [compressed_bits],
 * Fit pairs [lines] [8 L^2 counts of bit lengths 1..8], Fit residues [lines] [256 L counts]: csrc/mpc_fit.h) are plain uint64 sums, so ranks may all-reduce them
 * directly: mpc_stats_copy_raw_device enqueues an asynchronous device-to-device copy of
 * the raw_len words into d_dst on hip_stream (after everything already enqueued there),
 * and mpc_stats_from_raw turns such an array -- on the host, e.g. after the all-reduce --
 * into the statistics vector described above (merged-in host statistics not included; SC2 takes [0], [1], [3] and
 * [4], which the host counts, from this handle).  A Pattern handle covers ONE GPU: its set is per device, so T and [21] of
 * two handles that each saw a part of a trace do not add up to those of the whole trace; every other entry does. */
int mpc_stats_raw_len(const mpc_handle *h, uint64_t *raw_len);
int mpc_stats_copy_raw_device(mpc_handle *h, void *d_dst, void *hip_stream);
int mpc_stats_from_raw(const mpc_handle *h, const uint64_t *raw, size_t raw_len, uint64_t *vec, size_t n);
int mpc_stats_reset(mpc_handle *h);

/* ---- configuration check without a device --------------------------------
 * Parses and validates a VPC configuration exactly as mpc_create_vpc does and
 * writes a JSON description (line size, modules, id bits, which kernel path the
 * configuration maps to and why, whether the module sequence has an unrolled
 * instantiation or runs in the fast kernel's run-time module loop; "needs" / "runtime_only" and, per prediction module of a
 * fast plan, "kernel_base" / "kernel_shift" / "kernel_diff" / "base_form": what the planned kernel reads and does for every
 * byte, decoded from the kernel's own tables -- some 2 KiB per module at 128-byte lines) into out[cap].  Touches no HIP API.  Returns
 * 0, or the negative code mpc_create_vpc would return ({"error": ...}).     */
int mpc_config_describe(const char *config_json_text, char *out, size_t cap);

/* ---- file streaming (replaces trace::LoaderNPY, LoaderNPY.cpp:14-54) -----
 * Reads a C-order uint8 [N, L] .npy file in chunks straight into the pinned
 * staging buffers and evaluates rows [first_row, first_row+n_rows) clipped to
 * the file; skip_last_row != 0 reproduces the reference driver, which never
 * compresses the final row (LoaderNPY.cpp:28-32 + main.cpp:240).
 * rows_done receives the number of rows evaluated.                          */
int mpc_compress_npy(mpc_handle *h, const char *npy_path, uint64_t first_row,
                     uint64_t n_rows, int skip_last_row, uint64_t *rows_done);
/* Header probe: shape of a 2-D uint8 .npy file. */
int mpc_npy_shape(const char *npy_path, uint64_t *n_rows, uint64_t *line_size);

/* ---- GPGPU-Sim ".log" traces (replaces trace::gpgpusim::LoaderGPGPU,
 *      LoaderGPGPU.cpp:26-55, 93-119, plus the driver's filter, main.cpp:222-224)
 * File: 1 byte key count (17), 17 x (6-byte key, 1-byte size), then requests of
 * 62 header bytes + req_size data bytes.  Every complete request is read; only
 * GLOBAL_ACC_R (0) and GLOBAL_ACC_W (4) requests are evaluated; an incomplete
 * trailing request is ignored.  The line size is the req_size of the first
 * request (GetCachelineSize, LoaderGPGPU.cpp:16-24) and must equal the handle's;
 * an evaluated request of another size is an error (MPC_E_INVAL).
 * requests_read / lines_done may be NULL.                                    */
int mpc_compress_gpgpusim_log(mpc_handle *h, const char *log_path, uint64_t *requests_read,
                              uint64_t *lines_done);
/* Header probe: req_size of the first request (0 for a trace without requests). */
int mpc_gpgpusim_log_line_size(const char *log_path, uint32_t *line_size);

/* ---- groups: several evaluators over one trace (replaces main.cpp:208-248 run once per algorithm) ----
 * The reference compares compressors by running its driver once per algorithm: the trace is loaded and walked again
 * for each.  A group is an ordered set of existing handles of ONE line size on ONE device that are fed together: a
 * chunk of the trace is staged once (the group owns its two pinned + device slots) and every member's launch follows
 * on the slot's stream, in member order.  Each member sees every line exactly as if it had been called alone and keeps
 * its own statistics: mpc_stats_get and everything else that takes the member's handle work as before.  BDI, FPC and
 * BPC members of 32-, 64- or 128-byte lines, when at least two of them are in the group, share one kernel that loads a
 * line once and evaluates all of them on it; every other member launches its own kernel (a C-Pack member too; a Pattern
 * member its own kernels: the analysis and the set passes) (mpc_group_form).
 * The group BORROWS the handles: destroy the group before its members.  A member stays usable on its own between group
 * calls.  One group is used from one thread at a time.                                                             */
typedef struct mpc_group mpc_group;
/* MPC_E_INVAL with a message (mpc_group_last_error(NULL)) for: no member, a NULL or repeated handle, members of
 * different line sizes, members on different devices.                                                              */
int mpc_group_create(mpc_handle *const *members, size_t n, mpc_group **out);
void mpc_group_destroy(mpc_group *g);
/* Last error text of this group (or of the last failed mpc_group_create if g==NULL). */
const char *mpc_group_last_error(const mpc_group *g);
/* One line of text, for logs and tests: which members share a kernel launch and which run their own, in member order,
 * e.g. "VPC: unrolled; BDI+FPC+BPC: one kernel; SC2: own kernel" (a VPC member: its mpc_kernel_form).               */
const char *mpc_group_form(const mpc_group *g);
/* mpc_compress_batch for every member.  size_bits_out / selected_out: arrays of one pointer per member, in member
 * order; the array itself or any entry may be NULL (per-line output buffers exist only for members that were asked
 * for theirs).  Calls of up to 512 lines are evaluated in place from one small pinned buffer: one launch per member
 * or per shared launch, one synchronisation.                                                                      */
int mpc_group_compress_batch(mpc_group *g, const uint8_t *lines, uint64_t n_lines,
                             uint16_t *const *size_bits_out, int8_t *const *selected_out);
/* mpc_compress_batch_device for every member: asynchronous on `hip_stream`, optional DEVICE output arrays per member. */
int mpc_group_compress_batch_device(mpc_group *g, const void *d_lines, uint64_t n_lines,
                                    uint16_t *const *d_size_bits_out, int8_t *const *d_selected_out, void *hip_stream);
/* mpc_compress_npy / mpc_compress_gpgpusim_log for every member: the file is read and staged once. */
int mpc_group_compress_npy(mpc_group *g, const char *npy_path, uint64_t first_row, uint64_t n_rows,
                           int skip_last_row, uint64_t *rows_done);
int mpc_group_compress_gpgpusim_log(mpc_group *g, const char *log_path, uint64_t *requests_read, uint64_t *lines_done);
/* Waits for the group's slots and for the whole device (mpc_sync). */
int mpc_group_sync(mpc_group *g);

/* ---- size accounting: per-evaluator histograms of the per-line sizes, the per-line best-of of a group, sectors ----
 * Additive and off by default; declared in a header of its own, next to this one, which needs the two handle types
 * above.  MPC_ABI_VERSION, the statistics vectors, the raw layouts and mpc_info are unchanged by it.                */
#ifdef __cplusplus
}
#endif
#include "mpc_hip_sizes.h"
/* ---- per-class accounting: an evaluator's lines, bits and sector counts broken down by a class byte per line ----
 * Additive and off by default as well, in a header of its own for the same reason.                                  */
#include "mpc_hip_classes.h"
/* ---- pack accounting: the sectors that blocks of N consecutive lines occupy when they are packed and rounded once ----
 * Additive and off by default as well, in a header of its own for the same reason.                                  */
#include "mpc_hip_pack.h"
/* ---- image accounting: the latest size per line address, and the sectors that address-aligned blocks of it occupy ----
 * Additive and off by default as well, in a header of its own for the same reason.                                  */
#include "mpc_hip_image.h"
/* ---- rewrite accounting: the sequence of sizes per line address -- transitions between size classes, latest and peak ----
 * Additive and off by default as well, in a header of its own for the same reason.                                  */
#include "mpc_hip_rewrite.h"
/* ---- snapshots: the bytes of the latest unit per address, written out as address-aligned lines of any line size ----
 * An object of its own next to handles and groups, in a header of its own for the same reason.                      */
#include "mpc_hip_snapshot.h"
#ifdef __cplusplus
extern "C" {
#endif

/* ---- measurement helpers (bench.py; not part of the evaluator) -----------
 * Synthetic device-resident traces of SURVEY.md 8d, generated on the GPU:
 * kind 0 zeros, 1 random u32, 2 fp32 sine, 3 mixed int/fp, 4 pointer qwords.
 * first_line offsets the global line index so shards are independent.       */
int mpc_synth_fill(void *d_lines, uint64_t n_lines, unsigned line_size, int kind,
                   uint64_t first_line, uint64_t seed, void *hip_stream);
/* Pure streaming read of `bytes` bytes (sum-reduce to one word): the measured
 * HBM read ceiling on the same buffer.                                      */
int mpc_read_bandwidth_probe(const void *d_buf, uint64_t bytes, void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* MPC_HIP_H */
