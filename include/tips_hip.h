/*
 * tips_hip.h — C-ABI of libtips_hip.so, the MI355X-native gradient-bucket
 * reduction path behind TiPS's collective-allreduce API.
 *
 * Plain C: pointers, sizes, ints. No torch / TF / HIP types in any signature
 * (streams travel as `void*` = hipStream_t, NULL = the legacy default stream).
 * No exception crosses this boundary: every data-path call returns an int
 * status (TIPS_OK = 0, negative = error) and tips_last_error() returns the
 * message of the calling thread's last failure.
 *
 * Which reference interface each entry point replaces is cited per symbol.
 * Reference = Superjomn/TiPS.
 */
#ifndef TIPS_HIP_H_
#define TIPS_HIP_H_

#include <stdbool.h>
#include <stdint.h>

#if defined(__GNUC__)
#define TIPS_API __attribute__((visibility("default")))
#else
#define TIPS_API
#endif

#ifdef __cplusplus
extern "C" {
#endif

/* dtype codes: values 0-3 are message::DataType (tips/core/message/
 * collective_messages.fbs:17-23: TF_FLOAT32=0, TF_FLOAT64=1, TF_INT32=2,
 * TF_INT64=3). 4 and 5 are new in this build (the reference has no 16-bit
 * allreduce). */
enum tips_dtype {
  TIPS_FLOAT32 = 0,
  TIPS_FLOAT64 = 1,
  TIPS_INT32 = 2,
  TIPS_INT64 = 3,
  TIPS_FLOAT16 = 4,
  TIPS_BFLOAT16 = 5,
};

/* reduction codes = CollectiveOpKind (tips/core/collective/utils.h:21-25).
 * The reference only ever issues SUM (coordinator.cc:256-274), and tips_allreduce /
 * tips_allreduce_checked keep answering MAX/MIN with TIPS_ERR_UNSUPPORTED. MAX and MIN are
 * computed by the calls that take an op: tips_bucket_reduce, tips_multi_reduce and
 * tips_allreduce_op (below, "MAX and MIN"). */
enum tips_op {
  TIPS_OP_SUM = 0,
  TIPS_OP_MAX = 1,
  TIPS_OP_MIN = 2,
};

/* status codes (the reference returns tensorflow::Status, utils.h:66) */
enum tips_status {
  TIPS_OK = 0,
  TIPS_ERR_INVALID_ARG = -1,
  TIPS_ERR_NOT_INITIALIZED = -2,
  TIPS_ERR_HIP = -3,
  TIPS_ERR_RCCL = -4,
  TIPS_ERR_UNSUPPORTED = -5,
  TIPS_ERR_BOOTSTRAP = -6,
  TIPS_ERR_MISMATCH = -7,
};

/* allreduce algorithms (tips_set_algorithm). */
enum tips_algorithm {
  TIPS_ALGO_AUTO = -1,  /* oneshot for small buckets (<= TIPS_ONESHOT_BYTES, 256 KiB), else ring for
                           p <= 2 and direct otherwise; TIPS_ALGO env overrides */
  TIPS_ALGO_RING = 0,   /* RCCL send/recv ring, RS + AG, sub-chunk pipelined */
  TIPS_ALGO_DIRECT = 1, /* all-pairs RS over every xGMI link + p-input sum kernel + AG */
  TIPS_ALGO_RCCL = 2,   /* ncclAllReduce, kept as a comparison point only */
  TIPS_ALGO_ONESHOT = 3, /* whole bucket to every peer in one step + one p-input fold (small buckets) */
  TIPS_ALGO_PEER = 4,    /* direct's exchange by our own kernels through IPC-mapped peer memory (no RCCL):
                            push + rank-order fold + pull, phases ordered by a node-local shared-memory barrier.
                            Host-synchronous: a device-pointer call under PEER returns only after its push and
                            fold have run on every rank (each phase ends in a stream synchronize + barrier); only
                            the final pull is left queued on the caller's stream. */
  TIPS_ALGO_TUNE = 5,    /* measured choice: on the first call of each bucket-size class (a power of two), every
                            rank times ring and direct at several pipeline depths on scratch copies of the call's
                            input, the ranks agree on the slowest rank's times (one small ncclAllReduce MAX) and
                            all keep the fastest for that class; small buckets take AUTO's one-shot. The peer
                            schedule joins the candidates with TIPS_TUNE_PEER=1. tips_tuned_choice reports it. */
};

/* ---- lifecycle: same names and types as tips/core/operations.h:7-21 ---- */

/* Replaces tips_init (operations.cc:12-22). Collective over all ranks.
 * Reads RANK / WORLD_SIZE / LOCAL_RANK (torchrun) or OMPI_COMM_WORLD_* /
 * PMI_* (mpirun); WORLD_SIZE unset = one rank. For size > 1 the RCCL unique
 * id is exchanged over TCP: rank 0 listens on MASTER_ADDR:TIPS_BOOTSTRAP_PORT
 * (default MASTER_PORT + 17). Errors are reported by tips_last_error() and
 * tips_is_initialize() stays false (the reference CHECK-fails instead). */
TIPS_API void tips_init(void);
/* Replaces tips_shutdown (operations.cc:24-44). Safe to call twice. */
TIPS_API void tips_shutdown(void);
/* Replaces tips_is_initialize (operations.cc:46). */
TIPS_API bool tips_is_initialize(void);
/* Replace tips_size / tips_rank (operations.cc:48,50). -1 before init. */
TIPS_API int tips_size(void);
TIPS_API int tips_rank(void);

/* ---- lifecycle extensions (no reference counterpart) ---- */

/* Bytes of an RCCL unique id (128). */
TIPS_API int tips_unique_id_bytes(void);
/* Writes a fresh unique id into out[0..cap). Call on rank 0 only; returns bytes or <0. */
TIPS_API int tips_get_unique_id(void* out, int64_t cap);
/* Initialise with an id distributed by the caller (e.g. through a
 * torch.distributed store). device < 0: LOCAL_RANK % device count. */
TIPS_API int tips_init_rank(int rank, int size, int device, const void* unique_id, int64_t id_bytes);
/* The TCP exchange tips_init uses for the unique id, exposed for callers
 * that bootstrap themselves (and for CPU tests): rank 0's buf[0..bytes) is
 * delivered into every other rank's buf. Rank 0 listens on port; others
 * connect to host:port, retrying for up to timeout_s seconds. */
TIPS_API int tips_bootstrap_broadcast(int rank, int size, const char* host, int port, void* buf, int64_t bytes, int timeout_s);
/* Join counters of this process (both TCP joins: the bootstrap and the negotiation channel):
 * connections a joining rank dropped because they reached itself (TCP simultaneous open), and
 * connections rank 0 dropped because the joiner never confirmed them (it gave up waiting). */
TIPS_API int tips_net_stats(int64_t* self_connects_refused, int64_t* unconfirmed_joins_refused);
/* Diagnostics (no reference counterpart): one line on what the negotiation's threads are doing now
 * - the background thread's phase (waiting, exchanging cycle k, executing request i of a cycle's
 * list), the completion thread's (which request's device work it waits for), the request queues and
 * the names still waiting for other ranks. Never blocks on the library's locks: for a watchdog's
 * hang report. */
TIPS_API int tips_debug_state(char* out, int64_t cap);
/* Message of the calling thread's last failed call ("" if none). */
TIPS_API const char* tips_last_error(void);
/* Library version string. */
TIPS_API const char* tips_version(void);

/* ---- data path ---- */

/* dst[i] = a[i] + b[i] on the device: the per-chunk MPI_SUM local reduce
 * that MPI_Allreduce runs at every reduce-scatter step (reached from
 * AllreduceCpu<T>, tips/core/collective/utils.h:60-65). In-place (dst == a
 * or dst == b) allowed. count in elements (int64: lifts the reference's
 * int limit, utils.h:62). Device pointers only. Stream-ordered, async. */
TIPS_API int tips_bucket_sum(void* dst, const void* a, const void* b, int64_t count, int dtype, void* stream);

/* dst[i] = ((srcs[0][i] + srcs[1][i]) + srcs[2][i]) + ... (rank-order fold),
 * 1 <= nsrc <= 16. f16/bf16 partials are kept in fp32 and rounded once. */
TIPS_API int tips_multi_sum(void* dst, const void* const* srcs, int nsrc, int64_t count, int dtype, void* stream);

/* Replaces AllreduceCpu<T> (tips/core/collective/utils.h:52-67) and the
 * MPIAllreduce op's data path (tips/tensorflow/ops.cc:86-115):
 * out = SUM over ranks of in, out-of-place (in == out allowed).
 * Device pointers: stream-ordered, returns after enqueue (TIPS_ALGO_PEER excepted: it
 * blocks the host through its push and fold phases, see enum tips_algorithm).
 * Host pointers (both): staged through HBM, returns when out is written.
 * op must be TIPS_OP_SUM. */
TIPS_API int tips_allreduce(const void* in, void* out, int64_t count, int dtype, int op, void* stream);

/* ---- scaled forms: result = postscale * SUM over ranks of (prescale * x) ---- */

/* One definition for every call below (Scaled allreduce). Every input element is
 * multiplied by prescale exactly once, where a sum first reads it; every finished sum is multiplied
 * by postscale exactly once, where it is written. The arithmetic runs in the working type - fp32
 * for FLOAT32 / FLOAT16 / BFLOAT16, f64 for FLOAT64 - into which the factors are converted once on
 * the host; every multiply and every add is a separate IEEE operation (never a fused multiply-add),
 * and a kernel rounds to the storage type once, at its store. The factors sit inside the sum
 * kernels, so a scaled call moves the bytes of the plain one. Float dtypes only: an integer dtype
 * with a factor other than 1 returns TIPS_ERR_UNSUPPORTED; a factor that is not finite returns
 * TIPS_ERR_INVALID_ARG. With both factors 1 each call is its plain twin, bit for bit. The factors
 * must be the same on every rank (not validated). What the reference promises for
 * allreduce(op=Average, prescale_factor=, postscale_factor=) and leaves commented out at its C++
 * boundary (tips/tensorflow/__init__.py:82-87, :196). */

/* dst[i] = src[i] * factor (rounded once), dst == src allowed. Device pointers, stream-ordered. */
TIPS_API int tips_scale(void* dst, const void* src, int64_t count, int dtype, double factor, void* stream);
/* dst[i] = (a[i] * prescale + b[i] * prescale) * postscale: tips_bucket_sum's launch with the
 * factors inside it. In-place (dst == a or dst == b) allowed. */
TIPS_API int tips_bucket_sum_scaled(void* dst, const void* a, const void* b, int64_t count, int dtype, double prescale,
                                    double postscale, void* stream);
/* dst[i] = (((srcs[0][i] * prescale) + (srcs[1][i] * prescale)) + ...) * postscale, in source order:
 * tips_multi_sum's launch with the factors inside it, 1 <= nsrc <= 16. */
TIPS_API int tips_multi_sum_scaled(void* dst, const void* const* srcs, int nsrc, int64_t count, int dtype,
                                   double prescale, double postscale, void* stream);
/* out = postscale * SUM over ranks of (prescale * in): tips_allreduce (device or host pointers, the
 * pipelined host path included, in == out allowed) with the factors inside the schedule's sums - the
 * ring multiplies each rank's chunk by prescale in the step that first adds it and by postscale in
 * the step that completes it; direct and one-shot do both in their one fold. Under TIPS_ALGO_RCCL and
 * TIPS_ALGO_PEER the factors are applied unfused (a scaled copy of in into out, the in-place
 * allreduce, a scale of out). At one rank: the scaled copy. Routed through a running negotiation
 * as an ALLREDUCE request, like tips_allreduce. Never captured or replayed as a graph (TIPS_GRAPHS). */
TIPS_API int tips_allreduce_scaled(const void* in, void* out, int64_t count, int dtype, double prescale,
                                   double postscale, void* stream);

/* ---- MAX and MIN: the calls that take the reduction op ---- */

/* One definition for every call below (MAX and MIN). result[i] = the largest (TIPS_OP_MAX)
 * or smallest (TIPS_OP_MIN) of the operands' element i, in the storage type, exact: nothing is rounded.
 * INT32 / INT64 compare signed. FLOAT32 / FLOAT64 / FLOAT16 / BFLOAT16 follow IEEE 754-2019 maximum /
 * minimum: if any operand is a NaN the result is a NaN (payload and quiet bit unspecified), -0 < +0
 * (MAX(+0, -0) = +0, MIN(+0, -0) = -0), subnormals are kept, the infinities order as values. The
 * result does not depend on the order of the operands, so every schedule returns the same bits. There
 * is no scaled MAX / MIN. op outside {SUM, MAX, MIN} returns TIPS_ERR_INVALID_ARG; with TIPS_OP_SUM
 * each call is its plain twin (tips_bucket_sum, tips_multi_sum, tips_allreduce), bit for bit. */

/* dst[i] = op(a[i], b[i]): tips_bucket_sum's launch. In-place (dst == a or dst == b) allowed. */
TIPS_API int tips_bucket_reduce(void* dst, const void* a, const void* b, int64_t count, int dtype, int op, void* stream);
/* dst[i] = op over srcs[0..nsrc)[i], 1 <= nsrc <= 16 (one source: the copy): tips_multi_sum's launches. */
TIPS_API int tips_multi_reduce(void* dst, const void* const* srcs, int nsrc, int64_t count, int dtype, int op,
                               void* stream);
/* out = op over ranks of in: tips_allreduce (device pointers stream-ordered, or host pointers through
 * the staged and the pipelined host paths; in == out allowed) under ring, direct and one-shot, chosen
 * explicitly, by AUTO or by TUNE - the same plans, each sum replaced by the compare. At one rank: the
 * copy. Under TIPS_ALGO_RCCL: ncclAllReduce with ncclMax / ncclMin, whose own treatment of NaNs and
 * signed zeros applies. Under TIPS_ALGO_PEER MAX / MIN return TIPS_ERR_UNSUPPORTED on every rank, before
 * any exchange. Routed through a running negotiation as an ALLREDUCE request, like
 * tips_allreduce_scaled: the request record does not carry op, so op must be the same on every rank
 * and is not validated. Never captured or replayed as a graph (TIPS_GRAPHS). */
TIPS_API int tips_allreduce_op(const void* in, void* out, int64_t count, int dtype, int op, void* stream);

/* ---- sparse gradients: ordered row sums (Sparse allreduce) ---- */

/* One definition for the calls below. Inputs: values[n][row_elems] of one dtype, indices[n] (int64)
 * and a dense row count `rows`. Result: dense[rows][row_elems] with
 *     dense[j][:] = postscale * (e(x1) + e(x2) + ... + e(xk)),   e(x) = prescale * x
 * where x1 ... xk are the rows values[i][:] with indices[i] == j in ascending position i (for the
 * collective: ascending (rank, position)), folded left to right starting from the first row itself
 * (a lone -0 stays -0); a row no entry names is +0. The arithmetic runs in the working type - fp32
 * for FLOAT32 / FLOAT16 / BFLOAT16, f64 for FLOAT64, the integer type itself for INT32 / INT64 -
 * every multiply and add a separate IEEE operation, one rounding to the storage type at the store;
 * with both factors 1 there is no multiply at all. An integer dtype with a factor other than 1
 * returns TIPS_ERR_UNSUPPORTED, a factor that is not finite TIPS_ERR_INVALID_ARG; there is no MAX /
 * MIN form. An entry whose index is outside [0, rows) is skipped - it never reaches an address
 * computation - and counted (tips_sparse_stats). The result depends on nothing but the inputs: two
 * runs give the same bits, and so do one rank holding all the entries and p ranks holding them split
 * in rank order. Every pointer is a device pointer: a host pointer returns TIPS_ERR_UNSUPPORTED with
 * a message and is not staged. (The reference's tf.IndexedSlices branch, tips/tensorflow/
 * __init__.py:59-74, allgathers and leaves the sums to the consumer.) */

/* Bytes of workspace tips_rows_sum needs for `rows` dense rows and `n` entries:
 * 8 * (2 * rows + 2) + 16 * n (counts / offsets, cursors, placed and ordered entry ids). < 0 = error. */
TIPS_API int64_t tips_rows_sum_workspace(int64_t rows, int64_t n);
/* The local operation: dst[rows][row_elems] from this process's values / indices. Stream-ordered,
 * needs no tips_init (like tips_bucket_sum). Every row of dst is written exactly once (n == 0 writes
 * zeros); rows == 0 or row_elems == 0 is TIPS_OK with nothing launched. Negative sizes and a
 * workspace smaller than tips_rows_sum_workspace(rows, n) (or not 8-B aligned) return
 * TIPS_ERR_INVALID_ARG. dst, values, indices and workspace must not overlap. When every entry names
 * one row, ordering that row's entries costs O(n^2 / lanes of the device). */
TIPS_API int tips_rows_sum(void* dst, int64_t rows, int64_t row_elems, const void* values, const int64_t* indices,
                           int64_t n, int dtype, double prescale, double postscale, void* workspace,
                           int64_t workspace_bytes, void* stream);
/* The collective: dense_out[rows][row_elems] = the row sum over every rank's entries, the same on
 * every rank. The ranks first exchange {n, rows, row_elems, dtype} on the host (the gather behind
 * tips_allgather_i64): a difference in rows, row_elems or dtype returns TIPS_ERR_MISMATCH on every
 * rank before any device exchange. Indices and values then go through tips_allgatherv's path into
 * runtime scratch (ranks with n == 0 take part), and the row sum runs on the gathered arrays; at one
 * rank it runs straight on the caller's arrays, no copy. n may differ per rank; the factors must be
 * the same on every rank (not validated). Stream-ordered. Never captured or replayed as a graph.
 * While a negotiation runs (after the first named request) it returns TIPS_ERR_UNSUPPORTED: named
 * sparse requests are not implemented. */
TIPS_API int tips_sparse_allreduce(const void* values, const int64_t* indices, int64_t n, int64_t rows,
                                   int64_t row_elems, int dtype, double prescale, double postscale, void* dense_out,
                                   void* stream);
/* Counters of this process since the library was loaded: row sums launched (by either call above),
 * the entries they covered, and the entries skipped for an index outside [0, rows) - read back from
 * the device counter, so THIS CALL SYNCHRONISES THE DEVICE. Any pointer may be NULL (with
 * bad_indices NULL nothing is synchronised). */
TIPS_API int tips_sparse_stats(int64_t* calls, int64_t* entries, int64_t* bad_indices);

/* ---- Adasum (Adasum allreduce) ---- */

/* One definition for the calls below. A call reduces a list of SEGMENTS; a segment is one tensor, and
 * a single-tensor call has one. For two operands a and b holding the same segments, for each segment
 * s independently:
 *     d  = SUM a_i b_i    na = SUM a_i a_i    nb = SUM b_i b_i       (over the elements of s, in f64)
 *     ca = (na > 0) ? 1.0 - 0.5 (d / na) : 1.0                       (f64, every operation a separate IEEE op)
 *     cb = (nb > 0) ? 1.0 - 0.5 (d / nb) : 1.0
 *     out_i = round_S( fl_W( fl_W(ca_W a_i) + fl_W(cb_W b_i) ) )
 * W is the working type - fp32 for FLOAT32 / FLOAT16 / BFLOAT16, f64 for FLOAT64 - ca_W / cb_W the
 * coefficients rounded once from f64 to W, S the storage type: one rounding at the store. The
 * threshold is exact zero (this project's definition). Non-finite values get no special handling: a
 * NaN or an infinity anywhere in a segment of either operand makes that segment's whole result NaN;
 * other segments are unaffected. The three sums are accumulated in f64 in an order that is a function
 * of the segment's length and the dtype alone (DESIGN.md writes it down): alignment, the segment's
 * place in the buffer, its neighbours, the grid and the schedule change no bit, and two runs give the
 * same bits. Across p ranks, p a power of two, the result is the binary tree by recursive doubling:
 * at level k = 0 ... log2(p) - 1 rank r pairs with rank r XOR 2^k, a = the value of the partner
 * whose bit k is clear, b = the other's; both compute the same pair, so every rank ends with the
 * same bits; 16-bit storage rounds to storage at every level. p = 1 is the copy. Integer dtypes
 * return TIPS_ERR_UNSUPPORTED; there is no scaled Adasum; Adasum is not a tips_op and is never
 * captured or replayed as a graph. Every pointer is a device pointer: a host pointer returns
 * TIPS_ERR_UNSUPPORTED and is not staged. */

/* Bytes of workspace tips_adasum_pair needs for `count` elements in `nseg` segments, whatever the
 * float dtype: 8 * (3 * (count / 4096 + nseg) + 2 * nseg) rounded up to 256 (3 doubles per 32 KiB
 * chunk of a segment, 2 coefficients per segment). < 0 = error. */
TIPS_API int64_t tips_adasum_workspace(int64_t count, int nseg);
/* The local operation: dst = ca a + cb b over nseg segments that lie back to back in dst, a and b
 * (seg_counts[i] elements each, host array; their sum is the buffers' length). Stream-ordered, needs
 * no tips_init (like tips_bucket_sum and tips_rows_sum). dst may be a or b; otherwise the buffers and
 * the workspace must not overlap. Negative sizes and a workspace smaller than
 * tips_adasum_workspace(total, nseg) (or not 8-B aligned) return TIPS_ERR_INVALID_ARG, an integer
 * dtype TIPS_ERR_UNSUPPORTED; a total of 0 is TIPS_OK with nothing launched, and a segment of length 0
 * is legal and writes nothing. A list of more than one segment is uploaded as a table the first time
 * its counts are seen (that call synchronises with the device) and reused afterwards. */
TIPS_API int tips_adasum_pair(void* dst, const void* a, const void* b, const int64_t* seg_counts, int nseg, int dtype,
                              void* workspace, int64_t workspace_bytes, void* stream);
/* The collective over one tensor (one segment), out of place or in place (in == out),
 * stream-ordered: per level one RCCL send / recv of the whole buffer with the partner into runtime
 * scratch, then the pair on the same stream. The ranks first compare {tensors, elements, dtype, a hash
 * of the counts} on the host (the gather behind tips_allgather_i64): a difference returns
 * TIPS_ERR_MISMATCH on every rank before any device exchange. A rank count that is no power of two
 * returns TIPS_ERR_UNSUPPORTED on every rank, as does TIPS_ALGO_PEER; every other algorithm setting
 * is ignored (Adasum has its one schedule). While a negotiation runs (after the first named request)
 * it returns TIPS_ERR_UNSUPPORTED: named Adasum requests are not implemented. */
TIPS_API int tips_allreduce_adasum(const void* in, void* out, int64_t count, int dtype, void* stream);
/* The collective over a list: the n tensors are packed into `flat` at tips_fused_layout's offsets (the
 * pack launch of tips_fused_allreduce_flat), and the levels run over the whole flat buffer with one
 * segment per tensor - the padding between tensors travels with the buffer and is never part of a
 * segment. The same checks and refusals as tips_allreduce_adasum. */
TIPS_API int tips_fused_allreduce_adasum_flat(const void* const* ins, const int64_t* counts, int n, int dtype,
                                              void* flat, void* stream);

/* ---- MXFP8 wire (MXFP8 wire compression) ---- */

/* One definition for the calls below. The operand is a list of FLOAT32 device tensors laid out as
 * tips_fused_layout(counts, n, TIPS_FLOAT32, offsets) says (a single tensor is a list of one);
 * E = flat bytes / 4 elements. A BLOCK is 32 consecutive elements of that flat layout; tensors start
 * on multiples of 64 elements, so no block straddles two tensors, and a tensor's last block may be
 * partial: positions that hold no tensor element count as +0. The WIRE BUFFER of E elements holds one
 * payload byte per element (OCP e4m3fn) at byte i and one scale byte per block at byte
 * round_up(E, 256) + i / 32; it is round_up(E, 256) + round_up(E / 32, 256) bytes (tips_mxfp8_wire_bytes).
 *   Quantise, per block x_0 ... x_31: (1) any NaN or +-Inf poisons the block: scale byte 0xFF, all 32
 * payload bytes 0x7F, no other block affected. (2) Otherwise amax = max |x_j| with f32 biased exponent
 * be and fraction fr gives e = max(be, 1) - 127, s = e - 8 + (fr > 0x600000 ? 1 : 0) clamped to
 * [-127, 119], s = -127 for amax == 0; the scale byte is s + 127 (0 ... 246). (3) v_j = x_j * 2^-s as one
 * f32 multiply, |v_j| clamped to 448 (which binds only for amax > 448 * 2^119), rounded to nearest
 * even onto the e4m3fn grid, the sign kept (-0 -> 0x80). (4) Every payload and scale byte of the wire
 * buffer is written, padding positions and alignment tails as zeros with scale byte 0.
 *   Dequantise: y = decode_e4m3fn(byte) * 2^(scale byte - 127), one IEEE f32 multiply for every scale
 * byte 0 ... 254 (subnormals honoured, overflow to +-Inf); scale byte 255, and the payload codes 0x7F /
 * 0xFF, give NaN. With factor != 1 one further f32 multiply y * (float)factor follows. Every NaN is
 * written as 0x7FC00000.
 *   Fold of sources 0 ... k-1 over a block: every source dequantised (factor 1), acc = ((y0 + y1) + y2)
 * + ... as separate f32 adds in source order, then acc quantised: a poisoned source block or a sum
 * that is not finite poisons the result block by rule (1).
 *   Collective over ranks 0 ... p-1: result = dequantise(quantise(fold in rank order of quantise(x_r)),
 * factor): every rank decodes the same bytes, so every rank gets the same bits on every run; p = 1 is
 * the round trip dequantise(quantise(x)). A block with amax below 2^-137 decodes to zeros, one with
 * amax above 448 * 2^119 saturates its largest elements. Every pointer is a device pointer: a host
 * pointer returns TIPS_ERR_UNSUPPORTED and is not staged; tensors are 4-B aligned, wire buffers 16-B. */

/* Bytes of the wire buffer of `flat_elems` elements; *scales_offset (may be NULL) = the first scale
 * byte's offset, round_up(flat_elems, 256). Pure host. < 0 = error. */
TIPS_API int64_t tips_mxfp8_wire_bytes(int64_t flat_elems, int64_t* scales_offset);
/* The three local operations: stream-ordered, no tips_init needed (like tips_bucket_sum). Negative
 * sizes, nsrc outside 1 ... 16, a block range outside the buffer and a factor that is not a finite
 * float return TIPS_ERR_INVALID_ARG; a total of 0 elements (or 0 blocks) is TIPS_OK with nothing
 * launched, and an empty tensor inside a list is legal. `wire` must not overlap the tensors.
 * tips_mxfp8_quantize writes the whole wire buffer of the list ins[0 .. n). tips_mxfp8_fold writes
 * blocks [block_begin, block_begin + block_count) of dst_wire - payload and scale bytes, nothing
 * else - from the same blocks of the nsrc source wire buffers of flat_elems elements each; dst_wire
 * may be one of its sources. tips_mxfp8_dequantize writes the tensors outs[0 .. n) (their own
 * elements only) from the list's wire buffer. */
TIPS_API int tips_mxfp8_quantize(const void* const* ins, const int64_t* counts, int n, void* wire, void* stream);
TIPS_API int tips_mxfp8_fold(void* dst_wire, const void* const* src_wires, int nsrc, int64_t flat_elems,
                             int64_t block_begin, int64_t block_count, void* stream);
TIPS_API int tips_mxfp8_dequantize(void* const* outs, const int64_t* counts, int n, const void* wire, double factor,
                                   void* stream);
/* The collective over one tensor, out of place or in place (in == out), ordered on the caller's
 * stream: quantise into runtime scratch; the blocks cut into p contiguous chunks of whole blocks (a
 * function of (E, p) alone, payload chunks 256-B aligned); one RCCL group sends chunk q to rank q and
 * receives every peer's chunk `rank`; the fold of the p sources in rank order; one group gathers the
 * reduced chunks; dequantise with `factor`. The ranks first compare {tensors, elements, a hash of the
 * counts} on the host (the gather behind tips_allgather_i64): a difference returns TIPS_ERR_MISMATCH
 * on every rank before any device exchange. More than 16 ranks, TIPS_ALGO_PEER, a stream that is
 * being captured, and a running negotiation (named MXFP8 requests are not implemented) return
 * TIPS_ERR_UNSUPPORTED; every other algorithm setting is ignored. */
TIPS_API int tips_allreduce_mxfp8(const void* in, void* out, int64_t count, double factor, void* stream);
/* The collective over a list: tensor i's result at tips_fused_layout's offset i of `flat` (the
 * padding between tensors is not written). The same checks and refusals as tips_allreduce_mxfp8. */
TIPS_API int tips_fused_allreduce_mxfp8_flat(const void* const* ins, const int64_t* counts, int n, void* flat,
                                             double factor, void* stream);

/* ---- MXFP8 error feedback (MXFP8 error feedback) ---- */

/* The MXFP8 wire with a residual carried from one step to the next: each step keeps what its
 * quantisers dropped and adds it to the next step's input, so that what T steps deliver differs from
 * the true sum by one bounded residual, not by T roundings. Layout, block, wire buffer, quantise rules
 * (1)-(4), dequantise and fold are those of the MXFP8 wire above. B = ceil(E / 32) blocks; p ranks;
 * chunk q = blocks [min(q * per, B), min((q + 1) * per, B)) with per = round_up(ceil(B / p), 8), the
 * collective's chunk map.
 *   STATE: one caller-owned device buffer of f32 per list, 16-B aligned, zeroed by the caller before its
 * first use, of tips_mxfp8_ef_bytes(E, p) = 4 * (round_up(E, 256) + 32 * per) bytes (per = 0 for p = 1).
 * Elements [0, round_up(E, 256)) are the SENDER RESIDUAL r at the flat layout's positions; the 32 * per
 * elements behind it are the OWNER RESIDUAL o of this rank's own chunk, element 0 at the chunk's first
 * element. The state depends on the counts, on p and on the rank: a caller that changes any of them
 * starts again from zeros.
 *   Quantise with feedback, per block: c_j = x_j + r_j (one IEEE f32 add, not contracted) at every
 * position that holds a tensor element; a position that holds none counts as c_j = +0, and its residual
 * is neither read nor written. If any c_j is NaN or +-Inf the block is poisoned by rule (1) and
 * r'_j = +0 for its tensor elements - the step is lost, and the residual never carries a non-finite
 * value into later steps: from a finite state every r' is finite. Otherwise the block of c is quantised
 * by rules (2)-(3), y_j = decode_e4m3fn(byte_j) * 2^(scale byte - 127) (the dequantise with factor 1)
 * and r'_j = c_j - y_j (one IEEE f32 subtract) is stored to r. Rule (4) holds: every byte of the wire
 * buffer is written. With an all-zero residual the wire bytes are those of tips_mxfp8_quantize except
 * that an input -0 becomes +0 (-0 + +0 = +0) and encodes as 0x00, not 0x80.
 *   Fold with feedback over sources 0 ... k-1 of a block: acc = ((y0 + y1) + y2) + ... as above, then
 * c_j = acc_j + o_j (one f32 add after the last source). Poison is judged on c (a poisoned source or an
 * overflowing sum reaches c as NaN or Inf): a poisoned block sets o'_j = +0; otherwise c is quantised
 * and o'_j = c_j - y_j stored. The fold knows no tensors: every position of a block is handled alike
 * (padding positions hold zeros on every source, so their residual stays +0).
 *   Collective: the schedule of tips_allreduce_mxfp8 with its quantise replaced by the feedback form on
 * r and the owner's fold by the feedback form on o; dequantise and `factor` unchanged - residuals are
 * in units of the unscaled sum. p = 1 uses r only: dequantise(quantise_ef(x, r)). A rank whose chunk is
 * empty launches no fold and leaves o alone. Every rank decodes the same bytes: the outputs are the
 * same bits on every rank and every run; the states differ per rank by construction. */

/* Bytes of the state of a list of `flat_elems` flat elements on `nranks` (1 ... 16) ranks. Pure host.
 * < 0 = error. */
TIPS_API int64_t tips_mxfp8_ef_bytes(int64_t flat_elems, int nranks);
/* The two local operations with feedback: stream-ordered, no tips_init needed; the checks of
 * tips_mxfp8_quantize / tips_mxfp8_fold all apply. `residual` is a 16-B aligned device pointer that
 * overlaps neither the tensors nor a wire buffer (TIPS_ERR_INVALID_ARG; host memory:
 * TIPS_ERR_UNSUPPORTED): for the quantise the sender residual, round_up(E, 256) floats; for the fold
 * 32 * block_count floats, element 0 belonging to block `block_begin`. */
TIPS_API int tips_mxfp8_quantize_ef(const void* const* ins, const int64_t* counts, int n, void* wire, void* residual,
                                    void* stream);
TIPS_API int tips_mxfp8_fold_ef(void* dst_wire, const void* const* src_wires, int nsrc, int64_t flat_elems,
                                int64_t block_begin, int64_t block_count, void* residual, void* stream);
/* The collectives with feedback over the state `ef` of `ef_bytes` bytes. The checks and refusals of
 * tips_allreduce_mxfp8 all apply; `ef` is checked like `residual` above, as this rank's own verdict:
 * it travels in the ranks' host record like a host pointer does, so every rank fails the call together
 * (TIPS_ERR_MISMATCH "refused its arguments" on the others). An ef_bytes below
 * tips_mxfp8_ef_bytes(E, size) - a state sized for another list or rank count - is such a verdict and
 * is TIPS_ERR_MISMATCH on its own rank too. The call kind is part of the compared record: a feedback
 * call paired with tips_allreduce_mxfp8 / tips_fused_allreduce_mxfp8_flat on another rank returns
 * TIPS_ERR_MISMATCH on every rank. A call that fails these checks leaves the state untouched. */
TIPS_API int tips_allreduce_mxfp8_ef(const void* in, void* out, int64_t count, double factor, void* ef, int64_t ef_bytes,
                                     void* stream);
TIPS_API int tips_fused_allreduce_mxfp8_ef_flat(const void* const* ins, const int64_t* counts, int n, void* flat,
                                                double factor, void* ef, int64_t ef_bytes, void* stream);

/* ---- reduce-scatter (Reduce-scatter) ---- */

/* One definition for the calls below. ROW SPLIT: a contiguous tensor of shape [rows, ...] with
 * row_elems = the product of its trailing dimensions (1 for a 1-D tensor) is split along dimension 0
 * as Horovod's reducescatter does: with base = rows / p and rem = rows % p, rank q owns
 * base + (q < rem) rows from row q * base + min(q, rem); a rank may own none. RESULT: rank q's output
 * for tensor i has its own rows; element k is, for TIPS_OP_SUM, post * (((pre * x_0[k]) + (pre * x_1[k]))
 * + ... + (pre * x_{p-1}[k])) with x_r rank r's slice q, ranks ascending, in the working type (fp32
 * for FLOAT32 / FLOAT16 / BFLOAT16, f64 for FLOAT64, the storage type for the integers), every multiply
 * and add a separate IEEE operation and one rounding at the store - tips_multi_sum_scaled's fold, with
 * both factors 1 tips_multi_sum's; for TIPS_OP_MAX / TIPS_OP_MIN the exact compare of
 * tips_multi_reduce, without factors. The same bits on every run, and bit for bit the slice of what the
 * direct allreduce computes from the same inputs. REGION q of a list of n tensors is the
 * concatenation of every tensor's slice q in list order, each non-empty slice at the next multiple of
 * 256 bytes, empty slices taking no space: a function of (rows[], row_elems[], dtype, p, q) alone.
 *   Checks of the three device calls: an unknown dtype or op, a factor that is not finite and MAX / MIN
 * with a factor other than 1 return TIPS_ERR_INVALID_ARG, an integer dtype with a factor other than 1
 * TIPS_ERR_UNSUPPORTED; negative sizes and null lists TIPS_ERR_INVALID_ARG. Every pointer is a device
 * pointer aligned to its element: the collectives answer a host pointer with TIPS_ERR_UNSUPPORTED
 * (nothing is staged); tips_reducescatter_fold, like tips_multi_sum, does not probe its pointers. */

/* Pure host: the rows rank `rank` of `nranks` owns of a [rows, ...] tensor; *begin (may be NULL) = its
 * first row. < 0 = error. */
TIPS_API int64_t tips_reducescatter_rows(int64_t rows, int nranks, int rank, int64_t* begin);
/* Pure host: the bytes of region `rank` (up to its last slice's last byte); offsets[i] (offsets may be
 * NULL) = the byte offset of tensor i's slice in it. < 0 = error. */
TIPS_API int64_t tips_reducescatter_layout(const int64_t* rows, const int64_t* row_elems, int n, int dtype, int nranks,
                                           int rank, int64_t* offsets);
/* The kernel alone: stream-ordered, no communication, no tips_init needed. outs[i][k] for k < counts[i]
 * = the fold over sources j < nsrc in ascending j, where source own_pos is own[i] and source
 * j != own_pos is (char*)stages[j] + offsets[i] (stages[own_pos] is ignored and may be NULL; stages
 * may be NULL when nsrc is 1, which is the - scaled - copy). nsrc outside 1 ... 16, own_pos outside
 * 0 ... nsrc - 1, an offset that is no multiple of 256, segments that do not ascend without overlap,
 * a stage that is not 16-B aligned and a null pointer of a non-empty segment return
 * TIPS_ERR_INVALID_ARG. A segment of 0 elements is legal and touches nothing. Outputs must overlap
 * neither the own slices nor the stages. */
TIPS_API int tips_reducescatter_fold(void* const* outs, const void* const* own, const int64_t* counts,
                                     const int64_t* offsets, int n, const void* const* stages, int nsrc, int own_pos,
                                     int dtype, int op, double prescale, double postscale, void* stream);
/* The collective over one tensor, out of place, ordered on the caller's stream: `in` holds
 * rows * row_elems elements, `out` this rank's rows of them. Slice q goes to rank q straight from `in`
 * and every peer's slice `rank` arrives in runtime scratch, all in one RCCL group; one launch folds
 * the p sources in rank order into `out`. The ranks first compare {tensors, elements, a hash of the
 * (rows, row_elems) list, dtype, op, the factors' bits} on the host (the gather behind
 * tips_allgather_i64): a difference returns TIPS_ERR_MISMATCH ("Mismatched reduce-scatter ...") on every
 * rank before any device exchange. This rank's verdict on its own arguments - the checks above, an
 * output that overlaps an input (TIPS_ERR_INVALID_ARG), a stream that is being captured
 * (TIPS_ERR_UNSUPPORTED) - travels in that record, so the other ranks return TIPS_ERR_MISMATCH "refused
 * its arguments" and nobody waits. More than 16 ranks, TIPS_ALGO_PEER and a running negotiation (named
 * reduce-scatter requests are not implemented) return TIPS_ERR_UNSUPPORTED; every other algorithm
 * setting is ignored. A total of 0 elements is TIPS_OK; a rank that owns no row takes part in the
 * exchange and launches nothing. One rank: the (scaled) copy. */
TIPS_API int tips_reducescatter(const void* in, void* out, int64_t rows, int64_t row_elems, int dtype, int op,
                                double prescale, double postscale, void* stream);
/* The collective over a list of n tensors of one dtype: region q, packed into runtime scratch (one
 * launch per 112 peer slices), goes to rank q in one RCCL group; the fold writes every outs[i] from the staged regions and
 * this rank's own slices of ins[i]. The same checks and refusals as tips_reducescatter. */
TIPS_API int tips_grouped_reducescatter(const void* const* ins, void* const* outs, const int64_t* rows,
                                        const int64_t* row_elems, int n, int dtype, int op, double prescale,
                                        double postscale, void* stream);

/* ---- MXFP8 reduce-scatter (MXFP8 reduce-scatter) ---- */

/* The reduce-scatter with the MXFP8 wire: every peer value is quantised once, the owner's own slice
 * not at all, and the owner folds in f32. The operand is a list of n contiguous FLOAT32 device tensors
 * [rows_i, ...] with row_elems_i, split along dimension 0 by the ROW SPLIT above.
 *   REGION q is the list of every tensor's slice q in list order, slice i of rows_i,q * row_elems_i
 * elements. Its flat layout is tips_fused_layout over those slice counts as TIPS_FLOAT32: every
 * non-empty slice starts on a multiple of 64 elements; E_q flat elements, a function of (rows[],
 * row_elems[], p, q) alone; an empty slice is an empty tensor of the list. WIRE q OF RANK r is exactly
 * the bytes tips_mxfp8_quantize produces for rank r's slices q under that layout (payload, scale bytes
 * and quantise rules (1)-(4) of the MXFP8 wire above).
 *   RESULT on rank q, for tensor i and element k of its slice, at flat position f = off_i + k of region q:
 *     y_r = x_q[i][k]                             for r == q (this rank's own float32, not quantised)
 *     y_r = dequantise(wire q of rank r)[f]       for r != q (the MXFP8 wire's dequantise, factor 1)
 *     acc = ((y_0 + y_1) + y_2) + ... + y_{p-1}   ranks ascending, separate IEEE f32 adds, not contracted
 *     out = acc if (float)factor == 1, acc * (float)factor otherwise (one more f32 multiply)
 * Every NaN is stored as 0x7FC00000. A poisoned peer block (scale byte 0xFF) makes every tensor element
 * of that block NaN on the owner and nothing outside it; a NaN or Inf in the owner's own slice touches
 * only its own element. The same bits on every run. One rank, and one source, quantise nothing: the
 * result is what tips_reducescatter_fold gives with one source, TIPS_OP_SUM, prescale 1 and
 * postscale = factor - the copy, or the scaled copy. Positions that hold no tensor element are never
 * written. The owner's slice stays raw because only the owner ever computes its shard: there is no
 * "same bytes on every rank" to keep, and a quantise pass and a p-th of the error are saved - so an
 * allgather of these shards is not what tips_allreduce_mxfp8 returns. */

/* Pure host: E_rank, the flat elements of region `rank`; offsets[i] (offsets may be NULL) = the flat
 * element offset of tensor i's slice (0 for an empty slice). < 0 = error. */
TIPS_API int64_t tips_reducescatter_mxfp8_layout(const int64_t* rows, const int64_t* row_elems, int n, int nranks, int rank,
                                                 int64_t* offsets);
/* The kernel alone: stream-ordered, no communication, no tips_init needed. The layout is
 * tips_fused_layout(counts, n, TIPS_FLOAT32); outs[i][k] for k < counts[i] is the RESULT above over
 * sources j < nsrc, where source own_pos is own[i] and source j != own_pos is the 16-B aligned wire
 * buffer wires[j] of that layout (wires[own_pos] is ignored; wires may be NULL when nsrc is 1). nsrc
 * outside 1 ... 16, own_pos outside 0 ... nsrc - 1, negative counts, a null pointer of a non-empty
 * tensor, a tensor that is not 4-B aligned, a wire that is null or not 16-B aligned and a factor that
 * is not a finite float return TIPS_ERR_INVALID_ARG. A total of 0 elements is TIPS_OK with nothing
 * launched. Like tips_reducescatter_fold it does not probe its pointers. Outputs must overlap neither
 * the own slices nor the wires. */
TIPS_API int tips_reducescatter_mxfp8_fold(void* const* outs, const void* const* own, const int64_t* counts, int n,
                                           const void* const* wires, int nsrc, int own_pos, double factor, void* stream);
/* The collective over one tensor, out of place, ordered on the caller's stream. The ranks first compare
 * {tensors, elements, a hash of the (rows, row_elems) list with the call kind folded in, the factor's
 * float bits} on the host, in a record of the plain reduce-scatter's length: a difference - a call
 * paired with tips_reducescatter / tips_grouped_reducescatter on another rank included - returns
 * TIPS_ERR_MISMATCH ("Mismatched MXFP8 reduce-scatter ...") on every rank before any device exchange.
 * This rank's verdict on its own arguments (the checks of tips_reducescatter: sizes, a host pointer,
 * alignment, an output over an input, a capturing stream, and the factor) travels in that record, so
 * the other ranks return TIPS_ERR_MISMATCH "refused its arguments" and nobody waits. Then the slices of
 * the p - 1 peer regions are quantised into runtime scratch (the own region is not), one RCCL group
 * sends region q's payload and scale bytes to rank q and receives every peer's region `rank`
 * (regions of no block are skipped on both sides), and the fold-dequantise writes `out`. More than 16
 * ranks, TIPS_ALGO_PEER and a running negotiation return TIPS_ERR_UNSUPPORTED. A total of 0 elements
 * returns after the record exchange; a rank that owns no row takes part in the exchange and launches
 * nothing. One rank: the (scaled) copy. */
TIPS_API int tips_reducescatter_mxfp8(const void* in, void* out, int64_t rows, int64_t row_elems, double factor,
                                      void* stream);
/* The collective over a list of n FLOAT32 tensors: one quantise over the peers' slices (a launch per
 * 48 of them), one RCCL group, one fold launch per 80 output tensors. The same checks and refusals. */
TIPS_API int tips_grouped_reducescatter_mxfp8(const void* const* ins, void* const* outs, const int64_t* rows,
                                              const int64_t* row_elems, int n, double factor, void* stream);

/* ---- control plane: cross-rank request validation ---- */

/* request types = message::RequestType (collective_messages.fbs:3-7) */
enum tips_request_type {
  TIPS_REQ_ALLREDUCE = 0,
  TIPS_REQ_ALLGATHER = 1,
  TIPS_REQ_BROADCAST = 2,
};
#define TIPS_MAX_DIMS 8
/* one request record: {request_type, dtype, ndim, dims[TIPS_MAX_DIMS]} */
#define TIPS_REQUEST_WORDS (3 + TIPS_MAX_DIMS)

/* Replaces ConstructResponseMessage (coordinator.cc:90-186) and
 * GatherFirstRankSizes (coordinator.cc:40-88): table holds p request records
 * (rank order); each is compared with rank 0's. Returns TIPS_OK, or
 * TIPS_ERR_MISMATCH with the reference's error text in tips_last_error()
 * ("Mismatch data types found: 0 vs 1.", "Mismatched allreduce tensor shapes:
 * [2,4] vs [2,3]", "Mismatched allgather tensor shapes: 1-th dimension 3 vs 4",
 * ...). Pure host function. */
TIPS_API int tips_check_requests(const int64_t* table, int p);

/* tips_allreduce preceded by that validation: the records of all ranks are
 * exchanged (one small RCCL allgather + host sync), so every rank reaches the
 * same verdict; on a mismatch no rank reduces. shape = the tensor's dims. */
TIPS_API int tips_allreduce_checked(const void* in, void* out, const int64_t* shape, int ndim, int dtype, int op, void* stream);

/* ---- the other collectives of the op surface ---- */

/* out[r*words + w] = values[w] of rank r (host memory, blocking; words <= 4096). */
TIPS_API int tips_allgather_i64(const int64_t* values, int words, int64_t* out);
/* Replaces BroadcastCpu (utils.h:130-134) / MPIBroadcast (ops.cc:214-286):
 * out = root's in on every rank (in == out allowed). Any root (the reference
 * only supports 0, ops.cc:219). Host or device pointers, as tips_allreduce. */
TIPS_API int tips_broadcast(const void* in, void* out, int64_t count, int dtype, int root, void* stream);
/* Replaces AllgathervCpu (utils.h:83-128) / MPIAllgather (ops.cc:156-212):
 * out = concatenation over ranks of in, rank r contributing counts[r]
 * elements (counts[rank] must equal count). Host or device pointers. */
TIPS_API int tips_allgatherv(const void* in, int64_t count, void* out, const int64_t* counts, int dtype, void* stream);

/* Page-lock a long-lived host buffer (hipHostRegister) so host-memory calls on
 * it take the asynchronous DMA path (pinned: 40 GiB/s vs 29 GiB/s pageable for
 * a 256 MiB bucket). The caller must unregister before freeing
 * the memory. */
TIPS_API int tips_host_register(void* ptr, int64_t bytes);
TIPS_API int tips_host_unregister(void* ptr);

/* Tensor fusion (no reference counterpart): allreduce n device
 * tensors in place, packed into buckets of at most the fusion threshold
 * (TIPS_FUSION_THRESHOLD bytes, default 64 MiB; tensors at or above it are
 * reduced on their own). One dtype for all. The bucket layout depends only on
 * counts, dtype and threshold, never on where the tensors lie, so every rank
 * pairs the same elements. Stream-ordered on `stream`: the pack / unpack launches
 * run on `stream` itself (the bucket allreduces at N > 1 on a library stream forked
 * from it and joined back). Calls from different streams are safe: the fused calls
 * form one chain (each ends with an event a call from another stream waits for),
 * since the fusion slots and pointer tables are shared.
 * Graph capture: a fused call made under stream capture must find its pointer table
 * built (the same call made once before the capture) and stays out of the chain. The
 * table it used is then kept for the life of the job - never refilled, reused or freed
 * - and so are the fusion slots it packs into, past a change of TIPS_FUSION_THRESHOLD
 * (new slots are allocated beside them; all are freed at tips_shutdown). The replays
 * share those slots with eager fused calls: order a replay with fused calls on other
 * streams yourself (launch it on the same stream, or join the streams), as for any
 * graph that uses a shared workspace. */
TIPS_API int tips_fused_allreduce(void* const* ptrs, const int64_t* counts, int n, int dtype, void* stream);
/* The same, out of place: outs[i] = SUM over ranks of ins[i] (ins[i] == outs[i]
 * allowed); the inputs are left unchanged. What the reference's per-gradient
 * allreduce loop returns (tips/tensorflow/__init__.py:203-222), fused. */
TIPS_API int tips_fused_allreduce_oop(const void* const* ins, void* const* outs, const int64_t* counts, int n,
                                      int dtype, void* stream);

/* Compression.fp16 fused into the buckets (tips/tensorflow/compression.py:49-66 cast per tensor
 * before and after the allreduce, __init__.py:81-88): n f32 device tensors in[i] -> out[i]
 * (in == out allowed) allreduced in `wire_dtype` (TIPS_FLOAT16 or TIPS_BFLOAT16). Each tensor is cast
 * to the wire type (round to nearest even) as it is packed into a fusion bucket, every bucket is
 * allreduced in the wire type (half the bytes on the links), and cast back to f32 as it is
 * unpacked: one pack and one unpack launch per bucket instead of two casts per tensor. The
 * results are those of the per-tensor compress -> allreduce -> decompress. At one rank: the round
 * trip through the wire type. dtype must be TIPS_FLOAT32 (else TIPS_ERR_UNSUPPORTED), device memory,
 * stream-ordered as tips_fused_allreduce; routed through the negotiation (announced with the wire
 * type) once one runs. */
TIPS_API int tips_fused_allreduce_cast(const void* const* ins, void* const* outs, const int64_t* counts, int n,
                                       int dtype, int wire_dtype, void* stream);
/* The byte offset of each tensor of a fused list in ONE flat buffer laid out as the fusion buckets
 * (offsets[i], 256-B aligned; may be NULL); returns the flat buffer's size in bytes (< 0 = error).
 * A pure host function of counts, dtype and TIPS_FUSION_THRESHOLD - the same on every rank. */
TIPS_API int64_t tips_fused_layout(const int64_t* counts, int n, int dtype, int64_t* offsets);
/* flat = SUM over ranks of ins, tensor i at offsets[i] of tips_fused_layout (device memory of its
 * size): each bucket is packed straight into its region of `flat` and allreduced there in place -
 * no fusion slot, no unpack (2 x the gradient bytes of HBM traffic instead of 4 x). What
 * allreduce_grads returns views of (the reference's per-gradient loop, __init__.py:203-222). Inputs
 * unchanged; padding bytes of `flat` unspecified. One rank: one copy launch. Stream-ordered. */
TIPS_API int tips_fused_allreduce_flat(const void* const* ins, const int64_t* counts, int n, int dtype, void* flat,
                                       void* stream);
/* tips_fused_allreduce_flat with the scale of tips_allreduce_scaled: the pack is unchanged and each
 * bucket's in-place allreduce carries the factors; at one rank the pack is followed by one in-place
 * scale of the flat buffer. What allreduce_grads(op=Average) runs under set_op_scaling. */
TIPS_API int tips_fused_allreduce_flat_scaled(const void* const* ins, const int64_t* counts, int n, int dtype,
                                              void* flat, double prescale, double postscale, void* stream);
/* Measurement entry (bench.py, tools/copy_sweep_balanced.py): the pack launch the fusion issues for
 * bucket `bucket` of this list's layout (copy_segs_kernel over the bucket's tiles), into `dst` (device
 * memory of the bucket's padded size), on `stream`. Returns the bytes of the tensors the bucket holds
 * (the launch reads and writes each once), or with bucket < 0 the number of buckets; < 0 = error.
 * Part of the fusion chain like the calls above, except that it leaves the chain's end event to be
 * recorded on `stream` by the next fused call from another stream (so launches queue back to back):
 * `stream` must still exist then. */
TIPS_API int64_t tips_fused_pack_bucket(const void* const* ins, const int64_t* counts, int n, int dtype, int bucket,
                                        void* dst, void* stream);
/* Fusion caches of this process: layouts built / found (a layout is a function of the counts only,
 * so fresh gradient tensors every step still hit), and per-call pointer tables built (uploaded) /
 * found. Any pointer may be NULL. */
TIPS_API int tips_fusion_stats(int64_t* layouts_built, int64_t* layout_hits, int64_t* tables_built,
                               int64_t* table_hits);
/* Host tensors (numpy / CPU framework tensors, pageable or page-locked): outs[i] = SUM over ranks of
 * ins[i]. The list is packed by the library's host threads (TIPS_HOST_THREADS, 8) into page-locked
 * pieces of one byte stream (TIPS_HOST_FUSED_PIECE_BYTES, 32 MiB, ramped from 2 MiB at both ends);
 * each piece runs H2D -> allreduce in HBM -> D2H pipelined on separate streams while the threads
 * pack the next and unpack the previous.
 * The layout depends on the counts only. Blocks until every out is written (the reference's op is a
 * CPU op, ops.cc:118; its per-gradient loop, __init__.py:212-222, fused). */
TIPS_API int tips_fused_allreduce_host(const void* const* ins, void* const* outs, const int64_t* counts, int n,
                                       int dtype);
/* The same into ONE host buffer laid out as tips_fused_layout (the device flat layout): tensor i's sum at
 * offsets[i] of `flat`. When `flat` is page-locked (tips_host_register) each piece's D2H lands in it
 * directly - no unpack at all; otherwise through a page-locked slot and one contiguous copy per piece.
 * What allreduce_grads returns views of for host gradients. Blocks until `flat` is written. */
TIPS_API int tips_fused_allreduce_host_flat(const void* const* ins, const int64_t* counts, int n, int dtype,
                                            void* flat);

/* ---- named, asynchronous allreduce with cross-rank negotiation ---- */

/* Replaces EnqueueTensorCollective + the coordinator's background loop
 * (coordinator.cc:223-241, 355-513): requests may be enqueued in any order on
 * different ranks. A background thread per rank agrees with rank 0 (TCP,
 * MASTER_ADDR:TIPS_NEGOTIATION_PORT, default MASTER_PORT + 19) which names
 * every rank has enqueued, validates them with ConstructResponseMessage's
 * rules and error text, and every rank reduces them in rank 0's
 * readiness order (as ready_to_reduce), on the stream passed here. Device pointers run
 * stream-ordered; host pointers (both in and out host, as the reference's MPIAllreduce is a CPU
 * op, ops.cc:118) run on the negotiation thread, staged through HBM like tips_allreduce's, and
 * are done when tips_wait returns. Returns a handle > 0, or a negative status. The first call starts the
 * thread (collective: every rank's first named request must come after the same synchronous
 * collectives - their number is compared at the join, and a difference fails every rank's start
 * with both numbers instead of pairing RCCL calls wrongly). tips_shutdown stops it (collective).
 * From then on every synchronous collective of this library (tips_allreduce, tips_allreduce_checked,
 * tips_broadcast, tips_allgatherv, tips_allgather_i64, the tips_fused_* calls), from any thread, is
 * routed through the same negotiation: announced as request "~sync.<k>" (k-th such call of the rank)
 * with its type, dtype and shape, checked by rank 0 like any request, and run on the negotiation
 * thread in rank 0's order - so a rank's RCCL calls are issued from one thread in one order, the same
 * on every rank, as the reference's coordinator issues every collective. A routed call returns when
 * its device work is queued on the caller's stream (host memory: when it is done), as a direct call.
 * Synchronous calls from several threads at once must still come in the same order on every rank. */
TIPS_API int64_t tips_enqueue_allreduce(const char* name, const void* in, void* out, int64_t count, int dtype,
                                        void* stream);
/* The same with the tensor's shape (ndim <= TIPS_MAX_DIMS; ndim 0 = a scalar, announced as
 * shape [1] as CreateNoEmptyTfShape does, coordinator.cc:212-221): rank 0 validates shapes
 * with ConstructResponseMessage's rule and text (coordinator.cc:129-146), so a [2,4] request
 * on one rank and [4,2] on another fails on every rank with "Mismatched allreduce tensor
 * shapes: [2,4] vs [4,2]" although the element counts agree. tips_enqueue_allreduce
 * announces shape [count]. */
TIPS_API int64_t tips_enqueue_allreduce_shaped(const char* name, const void* in, void* out, const int64_t* shape,
                                               int ndim, int dtype, void* stream);
/* 1 = done (handle released), 0 = pending, < 0 = error (message in tips_last_error). */
TIPS_API int tips_poll(int64_t handle);
/* Blocks until the request is reduced (TIPS_OK, handle released) or failed (< 0). */
TIPS_API int tips_wait(int64_t handle);
/* n named requests in one call (what a framework's gradient hook hands over at once):
 * handles[i] = tips_enqueue_allreduce(names[i], ins[i], outs[i], counts[i], dtype, stream).
 * Returns TIPS_OK, or the first failure (its handles[i] < 0; the others are enqueued). */
TIPS_API int tips_enqueue_allreduce_n(const char* const* names, const void* const* ins, void* const* outs,
                                      const int64_t* counts, int n, int dtype, void* stream, int64_t* handles);
/* Shaped form of tips_enqueue_allreduce_n: tensor i has ndims[i] dims, taken in order from the
 * concatenated dims array (sum of ndims entries). */
TIPS_API int tips_enqueue_allreduce_shaped_n(const char* const* names, const void* const* ins, void* const* outs,
                                             const int* ndims, const int64_t* dims, int n, int dtype, void* stream,
                                             int64_t* handles);
/* tips_wait on each of n handles (handles <= 0 are skipped): TIPS_OK or the first failure. */
TIPS_API int tips_wait_n(const int64_t* handles, int n);
/* Completion callback of a named request (the reference's OpRecord::callback, ops.cc:107-110,
 * which sets the op's status and calls TF's done()): status TIPS_OK or a negative status, message
 * the failure's text ("" on success; valid during the call only). */
typedef void (*tips_done_fn)(void* ctx, int status, const char* message);
/* Register fn for the request `handle` (any of the three types): the library calls fn(ctx, status,
 * message) exactly once, from its completion thread, when the request has finished - for device
 * memory when its work on the device has completed - and releases the handle (tips_wait / tips_poll
 * on it then fail). A request that has already finished is called back at once (from that thread).
 * What an AsyncOpKernel body needs: enqueue, register, return; done() from the callback
 * (INTEGRATION.md §2). */
TIPS_API int tips_on_done(int64_t handle, tips_done_fn fn, void* ctx);
/* tips_enqueue_allreduce_shaped and tips_on_done in one call, as the reference enqueues one
 * OpRecord that carries its callback (EnqueueTensorCollective, coordinator.cc:223-241; CHECK(record.
 * callback)): one lock instead of two per request for an op body on many executor threads. Returns
 * the handle (> 0; it completes only through fn, and tips_wait / tips_poll / tips_on_done do not
 * know it) or < 0, in which case fn is never called. */
TIPS_API int64_t tips_enqueue_allreduce_cb(const char* name, const void* in, void* out, const int64_t* shape, int ndim,
                                           int dtype, void* stream, tips_done_fn fn, void* ctx);
/* Named broadcast through the same negotiation (the reference's MPIBroadcast op,
 * ops.cc:214-286 -> EnqueueTensorCollective(RequestType_BROADCAST); PerformCollectiveOp's
 * broadcast branch, coordinator.cc:275-295): rank 0 checks dtype and shape with
 * ConstructResponseMessage's rules and text ("Mismatched broadcast tensor shapes: ..."), and
 * that every rank names the same root. out = root's `in`, on `stream`, in rank 0's readiness
 * order with the other requests. (The reference's branch always broadcasts from rank 0 -
 * "root_rank should be passed in", coordinator.cc:280; here `root` is honoured.) */
TIPS_API int64_t tips_enqueue_broadcast(const char* name, const void* in, void* out, const int64_t* shape, int ndim,
                                        int dtype, int root, void* stream);
/* Output allocator of a named allgather: returns device memory of `bytes` (or NULL). Called
 * once, from the negotiation thread, when the output's size is known - as the reference's
 * PerformCollectiveOp allocates the op's output only then (context->allocate_output,
 * coordinator.cc:305-313). The caller owns what it returns. */
typedef void* (*tips_alloc_fn)(void* ctx, int64_t bytes);
/* Named allgather (MPIAllgather, ops.cc:156-212 -> RequestType_ALLGATHER): every rank's tensor
 * concatenated along dimension 0, in rank order. Rank 0 checks ndim and every dimension but
 * the first (GatherFirstRankSizes's rules and text, coordinator.cc:40-88) and sends every rank
 * the first dimensions; each rank then allocates its output through alloc(ctx, bytes), stores
 * the output's first dimension in *out_rows (valid once tips_wait / tips_poll report done) and
 * gathers on `stream`. ndim >= 1. A host `in` gets a host output: alloc must then return host memory. */
TIPS_API int64_t tips_enqueue_allgather(const char* name, const void* in, const int64_t* shape, int ndim, int dtype,
                                        void* stream, tips_alloc_fn alloc, void* ctx, int64_t* out_rows);

/* Select the allreduce algorithm (enum tips_algorithm). Returns TIPS_OK or an error. */
TIPS_API int tips_set_algorithm(int algo);
/* The algorithm currently selected (may be TIPS_ALGO_AUTO). */
TIPS_API int tips_get_algorithm(void);
/* The algorithm the current selection resolves to for a bucket of `bytes` on `nranks`. */
TIPS_API int tips_resolve_algorithm(int nranks, int64_t bytes);
/* Under TIPS_ALGO_TUNE: the schedule and pipeline depth this job measured for buckets of
 * `bytes`' size class. Returns 1 (and fills algo / depth) once that class has been tuned,
 * 0 before; < 0 on error. */
TIPS_API int tips_tuned_choice(int64_t bytes, int* algo, int* depth);
/* The same, with the number of transfer lanes the choice runs on: RCCL communicators split from
 * the job's, whose groups of consecutive plan steps are in flight together (1 = the comm stream
 * alone). TIPS_LANES sets it (the same on every rank) for an explicitly selected schedule. */
TIPS_API int tips_tuned_schedule(int64_t bytes, int* algo, int* depth, int* lanes);
/* Every candidate the tuner timed for `bytes`' size class: schedule, pipeline depth, lanes and
 * the slowest rank's ms per call (the numbers the choice was made on; the same on every rank).
 * Fills up to `cap` entries and returns how many candidates there were (0 before that class was
 * tuned; cap 0 asks the count), < 0 on error. */
TIPS_API int tips_tuned_timings(int64_t bytes, int* algos, int* depths, int* lanes, double* ms, int cap);
/* Replayed plans (TIPS_GRAPHS=1, opt-in; default 0): a ring / direct / one-shot call of at most
 * TIPS_GRAPH_MAX_BYTES (8 MiB: latency-bound buckets) made again on the same buffers (same
 * addresses and allocations) is captured once into a HIP graph and replayed with one launch;
 * streams, events and results are those of the eager steps. Needs ROCm >= 7.0 / RCCL >= 2.26
 * (torch's bundled runtime and /opt/rocm's 7.2 are both tested). Opt in only when no other thread
 * of the process issues work on the legacy null stream (hipMemcpy, hipMemset, launches on stream
 * 0, torch's default stream): such work invalidates a capture in progress on any stream, and RCCL
 * crashes inside the invalidated capture. Plans executed by the negotiation thread
 * (named requests, routed collectives) are never captured.
 * Reports this process's captures, replays and cached graphs.
 * A plan whose capture fails runs eagerly from then on; the others keep replaying.
 * Returns 0 (graphs on), 1 (3 failed captures turned them off for the job), 2 (off: not asked
 * for, or an older runtime), 3 (replays yielded: one bucket shape kept arriving at new addresses
 * after replays - TIPS_FRESH_WAIT_LIMIT host waits, 4 - so every plan now runs eagerly and no call
 * waits on the host), < 0 on error. */
TIPS_API int tips_graph_stats(int64_t* captured, int64_t* replayed, int64_t* cached);
/* The cost of keeping RCCL's order after replays: how many times an eager RCCL call (a larger
 * bucket, a fused call, a synchronous collective) found a replay still pending and blocked the
 * calling host thread until it had run (TIPS_REPLAY_HOST_ORDER, default 1), and the host time those
 * waits took in total (ns). Counts since tips_init. */
TIPS_API int tips_replay_order_stats(int64_t* host_waits, int64_t* host_wait_ns);


/* Pipeline shape the ring/direct schedules use for a bucket: depth = K
 * sub-chunks per chunk, sub_elems = elements in a (first) sub-chunk, i.e. the
 * size of one reduce-kernel launch (TIPS_PIPELINE_DEPTH, TIPS_MIN_SUBCHUNK_BYTES). */
TIPS_API int tips_schedule_shape(int64_t count, int p, int dtype, int* depth, int64_t* sub_elems);

/* Chunk partition the ring uses (element offsets), for tests. */
TIPS_API int tips_chunk_bounds(int64_t count, int p, int dtype, int c, int64_t* begin, int64_t* end);


#ifdef __cplusplus
}
#endif
#endif /* TIPS_HIP_H_ */
