/* kzg_mi355x.h -- C-ABI of libkzg_mi355x.so, the MI355X (gfx950) KZG segment prover.
 *
 * This is the drop-in boundary for the reference's prover seam: the reference miner talks to an external
 * prover process through `fourier.Client` (constructed at reference base/miner.py:73-84, used at
 * neurons/miner.py:39,48 and neurons/validator.py:59-104).  Each entry point below names the reference
 * interface it replaces.  The Python class zkp_subnet_amd.client.Client binds these through ctypes and
 * reproduces the Client method surface; INTEGRATION.md shows the binding a maintainer would add.
 *
 * Conventions
 *   - plain pointers and sizes only; the caller owns every buffer; the library copies in and out.
 *   - Fr  : 32 bytes big-endian, canonical (< r).  A non-canonical scalar fails the call (KZG_E_SCALAR).
 *   - G1  : affine x||y, 2 x 48 bytes big-endian (96 zero bytes = infinity), or the 48-byte ZCash
 *           compressed encoding for results.  Partial sums cross the ABI as 192 opaque bytes (XYZZ).
 *   - return 0 on success, negative kzg_status otherwise; kzg_last_error(ctx) gives the message.
 *     No exception or abort crosses the boundary.
 *   - one ctx = one GPU, and it is thread-safe: the reference's axon runs Miner.forward on worker threads
 *     (neurons/miner.py:106-135), so concurrent calls on one ctx each take one of four internal lanes (own HIP stream
 *     + workspace) and run concurrently on the GPU -- one request's sort and latency-bound tail hide under another's
 *     accumulate.  A fifth concurrent call waits for a lane.  (Re)loading the SRS and writing a resident slot are
 *     exclusive: they wait until the lanes are idle.  kzg_last_error reports the calling THREAD's last failure
 *     (ctypes releases the GIL during a call).
 *   - there is NO CPU fallback: every compute entry point fails with KZG_E_HIP when no gfx950 device works.
 */
#ifndef KZG_MI355X_H
#define KZG_MI355X_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct kzg_ctx kzg_ctx;

typedef enum {
    KZG_OK = 0,
    KZG_E_ARG = -1,     /* bad length / index / state */
    KZG_E_SCALAR = -2,  /* non-canonical Fr (>= r) */
    KZG_E_POINT = -3,   /* G1 input not reduced or not on the curve */
    KZG_E_HIP = -4,     /* HIP runtime failure or no usable device */
    KZG_E_NOMEM = -5,
    KZG_E_BUSY = -6,    /* an MSM ticket is outstanding (see kzg_msm_submit) */
    KZG_E_COMM = -7     /* RCCL: the library cannot be loaded, a collective call failed or timed out (kzg_comm_*) */
} kzg_status;

/* ---- lifecycle: replaces Client(port, bin, ...) + Client.start()/stop()  (reference base/miner.py:73-84,155,181) */
int kzg_create(int device_id, kzg_ctx** out);
void kzg_destroy(kzg_ctx* ctx);
const char* kzg_last_error(kzg_ctx* ctx); /* last failure of the calling thread; valid until its next failing call */
const char* kzg_version(void);
/* What the process around the context looks like, measured once by kzg_create.  The four lanes of a context overlap only
 * when the HIP runtime gives their streams different hardware queues: it has GPU_MAX_HW_QUEUES of them (default 4, read ONCE
 * when the runtime initialises) for every stream of the process.  The library never writes the environment (the axon's
 * threads may be reading it: neurons/miner.py:106-135 runs forward on worker threads): a launcher exports
 * GPU_MAX_HW_QUEUES=8 before the process's first HIP call (zkp_subnet_amd does at import), and this
 * call reports what the context actually got:
 *   out[0] lanes of a context (4)
 *   out[1] lanes measured to run concurrently: one spinning single-wave kernel per lane, the largest number alive at one
 *          instant -- out[0] when every lane has its own queue, 1 when they execute one after the other (results are the
 *          same either way; two requests in flight then gain nothing), 0 if the probe itself failed
 *   out[2] 1 if a HIP runtime was already initialised in the process when this library was loaded (an export made after
 *          that point came too late)
 *   out[3] GPU_MAX_HW_QUEUES as the environment showed it at kzg_create (0 = unset: the runtime's default) */
int kzg_runtime_info(kzg_ctx* ctx, int32_t out[4]);
/* window bits c for the signed-digit Pippenger tables; 0 = choose from the slice length.  Call before the SRS. */
int kzg_set_window(kzg_ctx* ctx, int c);
int kzg_get_window(kzg_ctx* ctx);
/* bit offsets of the windows actually in use: out[w] = first bit of window w, out[nwin] = 256; returns nwin */
int kzg_get_window_layout(kzg_ctx* ctx, int32_t* out_offsets, int max);

/* ---- SRS: replaces the prover's setup / precompute file loading (reference base/miner.py:75-84,
 *      utils/config.py:124-164).  The flat SRS holds 2^machines_scale-or-fewer worker slices of
 *      T = 2^(scale-machines_scale) points each, slice k at points [k*T, (k+1)*T).  Points stay resident
 *      ("cached SRS") together with their window multiples 2^off[w] P. */
int kzg_load_srs(kzg_ctx* ctx, const uint8_t* g1_affine_be96, uint64_t n_points, int scale, int machines_scale);
/* Same, from a ZCash-compressed file (48 bytes per point: flags 0x80 compressed | 0x40 infinity | 0x20 y-sign, x
 * big-endian) -- the reference's `uncompressed=False` setup files (base/miner.py:75-81, utils/config.py:131-150).
 * The y coordinates are recovered on the GPU (one Fp square root per point); a non-residue, x >= p or malformed flags
 * fail the load with KZG_E_POINT. */
int kzg_load_srs_compressed(kzg_ctx* ctx, const uint8_t* g1_c48, uint64_t n_points, int scale, int machines_scale);
/* The reference's own start path: Client(setup_path=...).start(scale, machines_scale) gives the prover a FILE
 * (base/miner.py:75-84; Makefile:63-74 starts mainnet from setup_24_8.uncompressed: 2^24 points, 1.6 GB).  The file
 * (96-byte records, or 48-byte compressed ones with compressed=1) is read with pread(2) straight into two pinned
 * tiles: host read, upload and GPU decode overlap, and a file truncated or replaced during the load is KZG_E_ARG (a
 * mapping would have raised SIGBUS).  All three loaders build the new tables aside and swap them in only
 * when the whole load has succeeded: after a failure (bad point, I/O, memory) the previously loaded SRS keeps serving. */
int kzg_load_srs_file(kzg_ctx* ctx, const char* path, int compressed, int scale, int machines_scale);
/* The same for ONE device of a host that spreads the worker rows over G GPUs (worker i on device i mod G: kzg_multi_*,
 * MultiDeviceClient): only the slices this context serves are read (pread of just those byte ranges), decoded, checked and
 * tabulated -- resident slice k = file slice first_slice + k * slice_stride, so worker index i = first_slice + k * slice_stride
 * is served as slice k.  Mainnet 24 / 8 on G devices: 34 / G GB of tables and ~1 / G of the start time per device instead of
 * the whole file on each (reference Makefile:63-74 starts one prover per process from the whole file: base/miner.py:75-81). */
int kzg_load_srs_file_slices(kzg_ctx* ctx, const char* path, int compressed, int scale, int machines_scale,
                             uint32_t first_slice, uint32_t slice_stride);
/* One contiguous SEGMENT of a flat SRS: file points [first_point, first_point + n_points) become the resident points
 * [0, n_points) of a single slice (machines_scale 0; n_points <= 2^scale, `scale` sizes the Pippenger window).  What device g
 * holds when ONE MSM is sharded by SRS segment over the GPUs of a host (kzg_multi_msm; BASELINE.json configs[3]). */
int kzg_load_srs_file_range(kzg_ctx* ctx, const char* path, int compressed, uint64_t first_point, uint64_t n_points, int scale);
/* seconds spent by the last successful load: [0] host copies into the pinned tiles, [1] host waiting for upload + decode
 * (decompression), [2] window-table build, [3] whole call */
int kzg_get_load_stats(kzg_ctx* ctx, double out_s[4]);
/* The loaders check every point: coordinates reduced, on the curve, AND in the prime-order subgroup G1 (E(Fp) has a
 * cofactor of ~2^126; the test is the endomorphism identity [z^2]P == -sigma(P), ~0.3 s for 2^24 points).  A failure is
 * KZG_E_POINT.  enable = 0 skips the membership part for a file whose provenance is already established: it applies to
 * the NEXT load only (whether that load succeeds or not) and the check is armed again afterwards -- a sticky switch
 * would silently cover later loads from caller memory too. */
int kzg_set_srs_subgroup_check(kzg_ctx* ctx, int enable);

/* synthetic SRS with known discrete logs (tests / benches; stands in for `fourier setup --generate-setup`,
 * reference tests/conftest.py:50-65): slice k, point j = [s0_k * tau^j] G.  s0_be32: n_slices x 32 bytes. */
int kzg_gen_srs(kzg_ctx* ctx, const uint8_t tau_be32[32], const uint8_t* s0_be32, uint32_t n_slices, int scale,
                int machines_scale);
uint64_t kzg_srs_points(kzg_ctx* ctx);
/* read back resident points: window w multiple of points [first, first+count) as affine be96 */
int kzg_srs_read(kzg_ctx* ctx, int w, uint64_t first, uint64_t count, uint8_t* out_be96);
int kzg_srs_read_compressed(kzg_ctx* ctx, int w, uint64_t first, uint64_t count, uint8_t* out_c48);

/* ---- hot path.  worker index i selects slice i of the resident SRS. */
/* replaces Client.worker_commit(i, poly)            (reference neurons/miner.py:38-45) */
int kzg_commit(kzg_ctx* ctx, uint32_t i, const uint8_t* row_be32, uint64_t T, int evaluation_form,
               uint8_t out_commitment48[48]);
/* replaces Client.worker_open(i, poly, x)           (reference neurons/miner.py:47-54) */
int kzg_open(kzg_ctx* ctx, uint32_t i, const uint8_t* row_be32, uint64_t T, int evaluation_form,
             const uint8_t alpha_be32[32], uint8_t out_eval32[32], uint8_t out_proof48[48]);
/* fused Miner.rpc_commit_and_open (reference neurons/miner.py:56-61): one upload, one IFFT, the two MSMs as one
 * batched pass (rows <= 2^18) or on two streams */
int kzg_commit_open(kzg_ctx* ctx, uint32_t i, const uint8_t* row_be32, uint64_t T, int evaluation_form,
                    const uint8_t alpha_be32[32], uint8_t out_commitment48[48], uint8_t out_eval32[32],
                    uint8_t out_proof48[48]);
/* Batched opening of k rows of worker i at ONE point alpha (the GWC batched opening a PLONK prover uses for the polynomials
 * of one sub-circuit): rows_be32 holds k rows of T elements each, row-major; out_commitments48[j] = kzg_commit(i, f_j),
 * out_evals32[j] = f_j(alpha), and ONE proof pi = MSM(U_i, (h - h(alpha)) / (X - alpha)) for h = sum_j gamma^j f_j --
 * exactly the proof of kzg_open(i, h, alpha).  k = 1 reproduces kzg_commit_open.  Verification (kzg_vk_verify_open_batch):
 *   e(sum_j gamma^j C_j - (sum_j gamma^j y_j) [L_i]_1, [1]_2) == e(pi, [tau_x - alpha]_2).
 * SOUNDNESS: gamma must be chosen by the verifier AFTER the commitments AND the evaluations y_j are fixed (a prover who
 * knows gamma before it commits to the y_j can pick two false ones whose errors cancel in the combination).  This call
 * returns the y_j and the proof together, so a Fiat-Shamir caller, who must hash the y_j before it derives gamma, cannot
 * use it as one step: it commits the rows as a set (kzg_rows_commit), hashes, gets the y_j from kzg_rows_eval, hashes them,
 * and proves with kzg_rows_open_lincomb.  The library takes gamma as an input, like alpha, and derives nothing: the
 * caller's protocol supplies both.  k = 0, k > KZG_MAX_BATCH_OPEN, alpha or gamma >= r and every worker-index / length
 * check of kzg_commit_open give KZG_E_ARG; the context keeps serving.  Rows up to 2^18 run as ONE MSM pass with k + 1
 * scalar sets (one sort, one bucket tree with k + 1 roots). */
#define KZG_MAX_BATCH_OPEN 16
int kzg_commit_open_batch(kzg_ctx* ctx, uint32_t i, uint32_t k, const uint8_t* rows_be32 /* k*T*32, row-major */,
                          uint64_t T, int evaluation_form, const uint8_t alpha_be32[32], const uint8_t gamma_be32[32],
                          uint8_t* out_commitments48 /* k*48 */, uint8_t* out_evals32 /* k*32 */, uint8_t out_proof48[48]);
/* Multi-point opening of k <= KZG_MAX_BATCH_OPEN rows of worker i at m <= KZG_MAX_OPEN_POINTS points (what a PLONK prover
 * opens per sub-circuit: every polynomial at zeta, the permutation accumulator and the shifted rows also at zeta * omega).
 * masks[p] (bit j = row j) names the rows opened at points_be32[p]; gammas_be32[p] is that point's challenge.  Returns the k
 * commitments, the evaluations y_{j,p} = f_j(alpha_p) of every masked pair (point-major, ascending j inside a point) and one
 * proof per point:
 *   pi_p = MSM(U_i, (h_p - h_p(alpha_p)) / (X - alpha_p)),  h_p = sum_t gamma_p^t f_{j_t}  over the masked rows
 *   j_0 < j_1 < ... of point p.
 * m = 1 with the full mask reproduces kzg_commit_open_batch byte for byte; two equal points each keep their own proof.
 * SOUNDNESS: as for kzg_commit_open_batch -- the alpha_p must be drawn AFTER the commitments are fixed, and the gamma_p
 * AFTER the commitments and the evaluations y_{j,p}; a Fiat-Shamir caller therefore goes through committed row sets,
 * kzg_rows_eval and kzg_rows_open_lincomb.  The library derives none of them.  k = 0, k > KZG_MAX_BATCH_OPEN, m = 0, m > KZG_MAX_OPEN_POINTS, a zero mask, a
 * mask bit >= k, an alpha_p or gamma_p >= r and every worker-index / length check of kzg_commit_open give KZG_E_ARG; the
 * context keeps serving.  The rows are uploaded and transformed once; rows up to 2^18 run as ONE MSM pass with k + m scalar
 * sets while the sort's key carries them (else as few passes as fit). */
#define KZG_MAX_OPEN_POINTS 4
int kzg_commit_open_multi(kzg_ctx* ctx, uint32_t i, uint32_t k, const uint8_t* rows_be32 /* k*T*32, row-major */, uint64_t T,
                          int evaluation_form, uint32_t m, const uint8_t* points_be32 /* m*32 */, const uint32_t* masks /* m */,
                          const uint8_t* gammas_be32 /* m*32 */, uint8_t* out_commitments48 /* k*48 */,
                          uint8_t* out_evals32 /* sum popcount(masks)*32 */, uint8_t* out_proofs48 /* m*48 */);
/* Committed row sets: commit k rows once, open them later -- the shape of a Fiat-Shamir prover, whose challenges are hashes
 * of commitments it has already published (commit the wire rows; derive a challenge, commit the accumulator; derive one,
 * commit the quotient pieces; derive zeta, open everything at zeta and the accumulator also at zeta * omega).
 * kzg_rows_commit: k in [1, KZG_MAX_BATCH_OPEN] rows of worker i, with the argument checks of kzg_commit_open_batch (each a
 * KZG_E_ARG).  out_commitments48[j] == kzg_commit(i, row j) byte for byte.  The set keeps the k coefficient rows on the
 * device under *out_handle (it remembers i and T).  More than KZG_MAX_ROW_SETS live sets: KZG_E_BUSY; a failed device
 * allocation: KZG_E_NOMEM.
 * kzg_rows_open: the rows of the n_handles sets, numbered by concatenating the sets' rows in the order of `handles` (a handle
 * may appear more than once; at most KZG_MAX_BATCH_OPEN rows in all), opened at m points under the rules of
 * kzg_commit_open_multi over those rows.  out_evals32 (its point-major layout) and out_proofs48 equal what
 * kzg_commit_open_multi writes for the concatenated rows, byte for byte, so kzg_vk_verify_open_multi checks them against the
 * concatenated commitments.  No upload, no INTT, no commitment MSM.  Sets of different workers or lengths, an unknown or
 * released handle and a set made stale by an SRS (re)load give KZG_E_ARG.  A set can be opened any number of times, also by
 * concurrent threads.
 * kzg_rows_release: frees the set; its handle then gives KZG_E_ARG to an open and to a second release.  Handles are never
 * reused within the process.  A release racing an open of the same set is safe: the open finishes with correct bytes and
 * the memory is reclaimed after it.  Any kzg_load_srs* / kzg_gen_srs makes every live set stale (its commitments belong to
 * the old SRS); its release still succeeds.  kzg_destroy frees every set.  After any error the context keeps serving.
 * kzg_rows_stats: out[0] live sets (stale ones included until released), out[1] the device bytes their rows hold.
 * SOUNDNESS: with sets the caller can fix and hash the commitments BEFORE it draws the points.  kzg_rows_open still takes
 * the gammas together with returning the evaluations, and the gammas must come AFTER the evaluations are fixed (see
 * kzg_commit_open_batch); a Fiat-Shamir caller uses kzg_rows_eval, hashes the evaluations, then kzg_rows_open_lincomb.
 * The library still derives no challenge. */
#define KZG_MAX_ROW_SETS 64   /* live sets per context */
int kzg_rows_commit(kzg_ctx* ctx, uint32_t i, uint32_t k, const uint8_t* rows_be32 /* k*T*32 */, uint64_t T,
                    int evaluation_form, uint8_t* out_commitments48 /* k*48 */, uint64_t* out_handle);
int kzg_rows_open(kzg_ctx* ctx, uint32_t n_handles, const uint64_t* handles, uint32_t m, const uint8_t* points_be32 /* m*32 */,
                  const uint32_t* masks /* m */, const uint8_t* gammas_be32 /* m*32 */,
                  uint8_t* out_evals32 /* sum popcount(masks)*32 */, uint8_t* out_proofs48 /* m*48 */);
int kzg_rows_release(kzg_ctx* ctx, uint64_t handle);
int kzg_rows_stats(kzg_ctx* ctx, uint64_t out_live_sets_bytes[2]);
/* Typed columns in, cells of resident rows back out: the two ends of a witness that otherwise never leaves the device.
 * kzg_rows_commit_typed: kzg_rows_commit whose k rows arrive one column each, as integers of their natural width instead of 32
 * big-endian bytes per cell.  Column c holds cols[c].count <= T cells at cols[c].data (host memory, any alignment; native
 * little-endian for the integer kinds, 32 big-endian bytes per cell for KZG_COL_BE32); cells [count, T) take fill_be32 (null:
 * 0).  A negative cell x of a signed kind is r - |x|.  The set, its handle, commitments, buffer contents and kzg_rows_stats
 * accounting are those of kzg_rows_commit on the same values written as be32 rows; only k * count * width bytes cross the
 * host link.  The checks of kzg_rows_commit on i, T and evaluation_form apply; k outside [1, KZG_MAX_BATCH_OPEN], an unknown
 * kind, count > T, a null data with count > 0, a KZG_COL_BE32 cell or a fill >= r: KZG_E_ARG, and no set is left behind.
 * kzg_rows_read: cells [first, first + count) of row `row` of the concatenated sets (numbered as in kzg_rows_open), as the
 * values on the domain (evaluation_form = 1: what was uploaded or built; T must be a power of two) or the coefficients
 * (evaluation_form = 0).  `kind` chooses the output: KZG_COL_BE32 writes 32 big-endian bytes per cell, an integer kind
 * native little-endian integers of its width, where a value >= r - 2^(w-1) reads as negative for the signed kinds.  A cell
 * that does not fit the kind is written as 0 and counted: out_overflow[0] = how many, out_overflow[1] = the smallest such
 * row index (UINT64_MAX: none); that is no error.  first + count > T, a row outside the concatenation, a quotient accumulator,
 * an unknown, released or stale handle: KZG_E_ARG.  count = 0 succeeds and writes nothing.  The sets are unchanged; reads
 * run beside opens of the same set, under the rules of kzg_rows_open for a release or an SRS load that races them. */
enum { KZG_COL_BE32 = 0, KZG_COL_U8, KZG_COL_U16, KZG_COL_U32, KZG_COL_U64, KZG_COL_I32, KZG_COL_I64 };
typedef struct {
    const void* data;         /* `count` cells */
    uint64_t count;           /* <= T */
    uint32_t kind;            /* KZG_COL_* */
    const uint8_t* fill_be32; /* 32 bytes, canonical; NULL: 0 */
} kzg_col;
int kzg_rows_commit_typed(kzg_ctx* ctx, uint32_t i, uint32_t k, const kzg_col* cols /* k */, uint64_t T, int evaluation_form,
                          uint8_t* out_commitments48 /* k*48 */, uint64_t* out_handle);
int kzg_rows_read(kzg_ctx* ctx, uint32_t n_handles, const uint64_t* handles, uint32_t row, uint64_t first, uint64_t count,
                  uint32_t kind, int evaluation_form, void* out /* count * width */, uint64_t out_overflow[2]);
/* Evaluate first, then open caller-weighted combinations: the two calls of a Fiat-Shamir opening round (PLONK round 5).
 *   1. kzg_rows_commit the sets; hash the commitments, derive zeta.
 *   2. kzg_rows_eval; hash the evaluations, derive v.
 *   3. compute the combination scalars on the host (the linearisation's c_j from the evaluations, v powers for the rest).
 *   4. kzg_rows_open_lincomb.
 * kzg_rows_eval: y_{j,p} = f_j(alpha_p) of every masked (row, point) pair of committed sets, no proof, no MSM.  Rows
 * numbered, masks, point checks, handle rules (unknown / released / stale / mixed worker or length -> KZG_E_ARG) and the
 * point-major output layout exactly as kzg_rows_open; out_evals32 equals kzg_rows_open's byte for byte for the same
 * points / masks.
 * kzg_rows_open_lincomb: one proof per point for a caller-weighted combination of the k concatenated rows:
 *   h_p = sum_j lambda_{p,j} f_j,  v_p = h_p(alpha_p),  pi_p = MSM(U_i, (h_p - v_p) / (X - alpha_p))
 * -- exactly kzg_open(i, h_p, alpha_p).  coeffs_be32: m x k canonical scalars, point-major; a zero coefficient leaves the row
 * out.  k must equal the rows of the concatenation; a coefficient or point >= r, a point whose k coefficients are all zero,
 * m = 0 or m > KZG_MAX_OPEN_POINTS -> KZG_E_ARG.  No pair evaluation, no commitment MSM: the combination, the m openings
 * and the m proof MSMs.  The verifier forms sum_j lambda_{p,j} C_j from commitments it already holds
 * (kzg_vk_verify_open_lincomb), so a linearisation polynomial is never committed.
 * Both are thread-safe like kzg_rows_open and follow its rules for a release or an SRS load that races them; after any
 * error the context keeps serving. */
int kzg_rows_eval(kzg_ctx* ctx, uint32_t n_handles, const uint64_t* handles, uint32_t m, const uint8_t* points_be32 /* m*32 */,
                  const uint32_t* masks /* m */, uint8_t* out_evals32 /* sum popcount(masks)*32 */);
int kzg_rows_open_lincomb(kzg_ctx* ctx, uint32_t n_handles, const uint64_t* handles, uint32_t k, uint32_t m,
                          const uint8_t* points_be32 /* m*32 */, const uint8_t* coeffs_be32 /* m*k*32 */,
                          uint8_t* out_values32 /* m*32 */, uint8_t* out_proofs48 /* m*48 */);
/* SHPLONK (BDFG20) multi-open over committed sets: ONE proof pair (W, pi) for k rows opened at any number of points, where the
 * GWC calls above return one proof per point.  Rows f_0 .. f_{k-1}: the concatenated rows of the handles' sets; points
 * alpha_0 .. alpha_{m-1}, pairwise distinct, P the set of all of them; masks[p] bit j set when row j is opened at alpha_p (the
 * convention of kzg_rows_eval), S_j = { p : bit j of masks[p] } row j's point set, Z_S = prod_{p in S} (X - alpha_p), r_j the
 * interpolant of f_j on S_j; c_0 .. c_{k-1} caller scalars (in halo2: products of powers of its challenges y and v).
 * Round A, kzg_rows_commit_shplonk -- a set built FROM sets:
 *   h = sum_{j : c_j != 0} c_j (f_j - r_j) / Z_{S_j}
 * is computed on the device (rows with equal S_j are combined first, then divided by one point after the other; no
 * evaluation, no interpolation), and committed as a new ONE-ROW set of the same worker and length: out_commitment48 = W
 * equals kzg_commit of h's coefficients (T of them, evaluation_form = 0) byte for byte, and *out_handle opens, evaluates,
 * combines, releases, goes stale and counts against KZG_MAX_ROW_SETS (KZG_E_BUSY; KZG_E_NOMEM on a failed allocation) like
 * any other.  No upload of anything row-sized, no evaluation returned.
 * Round B is host arithmetic and kzg_rows_open_lincomb: the caller hashes W, draws u outside P, and with
 *   lambda_j = c_j Z_{P \ S_j}(u)  (j < k),   lambda_k = -Z_P(u)
 * opens L = sum_j lambda_j f_j + lambda_k h -- the k rows followed by h -- at the single point u.  The call returns
 *   v = L(u) = sum_j c_j Z_{P \ S_j}(u) r_j(u)   and   pi = [(L - v) / (X - u)].
 * The proof is (W, pi): 96 bytes, two MSMs and (kzg_vk_verify_open_shplonk) two pairings whatever m is.
 * Handle rules as kzg_rows_commit_grand_product: a handle may repeat (its rows are numbered twice); unknown / released /
 * stale handles, mixed workers or lengths -> KZG_E_ARG; the source sets are only read; a release or an SRS load racing the
 * call behaves as for kzg_rows_open; thread-safe; after any error the context keeps serving.  KZG_E_ARG with a message that
 * names it: k != the rows of the concatenation; k = 0 or k > KZG_MAX_SHPLONK_ROWS; m = 0 or m > KZG_MAX_SHPLONK_POINTS; a
 * point or coefficient >= r; two equal points (unlike the GWC calls, where each point keeps its own proof); a mask bit >= k;
 * a row with c_j != 0 and an empty S_j; all c_j zero; some |S_j| >= T.  A row with c_j = 0 is left out, whatever its mask.
 * More than KZG_MAX_SHPLONK_ROWS opened rows compose by linearity: several round-A calls with the same points, their W (and
 * later their pi) summed with kzg_g1_sum_compressed and their v added; the library has no helper for that.
 * SOUNDNESS: the c_j must be drawn AFTER the commitments AND the evaluations of kzg_rows_eval are fixed, and u AFTER W.  The
 * library derives no challenge. */
#define KZG_MAX_SHPLONK_POINTS 8
#define KZG_MAX_SHPLONK_ROWS   (KZG_MAX_BATCH_OPEN - 1)    /* round B opens k + 1 rows */
int kzg_rows_commit_shplonk(kzg_ctx* ctx, uint32_t n_handles, const uint64_t* handles, uint32_t k, uint32_t m,
                            const uint8_t* points_be32 /* m*32 */, const uint32_t* masks /* m */,
                            const uint8_t* coeffs_be32 /* k*32 */, uint8_t out_commitment48[48], uint64_t* out_handle);
/* A set built FROM sets: the permutation grand product (PLONK round 2), computed and committed on the device from rows that
 * are already resident.  The wire rows a_0 .. a_{k-1} are the concatenated rows of the wire_handles sets, the permutation rows
 * sigma_0 .. sigma_{k-1} those of the sigma_handles sets.  With w the T-th root of unity of evaluation_form = 1 rows
 * (7^((r-1)/T), natural order), s_j = shifts[j] and t in [0, T):
 *   N_t = prod_j (a_j(w^t) + beta s_j w^t + gamma),   D_t = prod_j (a_j(w^t) + beta sigma_j(w^t) + gamma),
 *   z(w^0) = 1,  z(w^(t+1)) = z(w^t) N_t / D_t  (t < T - 1),   closing = prod_t N_t / prod_t D_t.
 * The call creates a new ONE-ROW set of the same worker and length holding z's coefficients, exactly as if z's T evaluations
 * had gone through kzg_rows_commit(i, 1, z, T, 1, ..): out_commitment48 equals that call's byte for byte and *out_handle opens,
 * evaluates, combines, releases, goes stale and counts against KZG_MAX_ROW_SETS (KZG_E_BUSY; KZG_E_NOMEM on a failed
 * allocation) like any other.  out_closing32 is what z(w^T) would be, canonical big-endian: 1 exactly when the product
 * closes.  The library does not judge it.  Nothing row-sized crosses the host link in either direction.
 * Handle lists follow kzg_rows_open: 1 .. KZG_MAX_BATCH_OPEN handles each, a handle may repeat, unknown / released / stale ->
 * KZG_E_ARG; each concatenation must hold exactly k rows, 1 <= k <= KZG_MAX_BATCH_OPEN; every set named must belong to one
 * worker and one (power-of-two) T; beta, gamma or a shift >= r -> KZG_E_ARG.  A zero denominator (some D_t = 0) leaves z
 * undefined: KZG_E_ARG with a message that says so, no set created.  The source sets are only read; a release or an SRS
 * load racing the call follows the rules of kzg_rows_open.  Thread-safe like every call; after any error the context keeps
 * serving.
 * SOUNDNESS: beta and gamma must be drawn AFTER the wire commitments are fixed (a prover who knows them before it commits
 * the wires can make a false permutation close).  The library derives no challenge and adds NO BLINDING: a blinded z has
 * degree >= T and does not fit a T-point slice; a caller who blinds pads its circuit below T and calls
 * kzg_rows_commit_grand_product_zk below, which fills the blinding rows. */
int kzg_rows_commit_grand_product(kzg_ctx* ctx, uint32_t n_wire_handles, const uint64_t* wire_handles,
                                  uint32_t n_sigma_handles, const uint64_t* sigma_handles, uint32_t k,
                                  const uint8_t* shifts_be32 /* k*32 */, const uint8_t beta_be32[32],
                                  const uint8_t gamma_be32[32], uint8_t out_commitment48[48], uint8_t out_closing32[32],
                                  uint64_t* out_handle);
/* A fourth set built FROM sets: the running sum of a log-derivative lookup argument (logUp), computed and committed on the
 * device from rows that are already resident.  The concatenated rows of the input_handles sets are the L * w rows f_{l,c},
 * lookup-major (l < L = n_lookups, c < w = width); those of the table_handles sets are the w table columns t_c; mult_handle
 * names a ONE-row set m, the multiplicities (how many input cells hit table row t).  With w_T the T-th root of unity of
 * evaluation_form = 1 rows (7^((r-1)/T), natural order) and t in [0, T):
 *   F_l(w_T^t) = sum_c theta^c f_{l,c}(w_T^t),   Tb(w_T^t) = sum_c theta^c t_c(w_T^t)        (theta unused when w = 1)
 *   term_t = sum_l 1 / (beta + F_l(w_T^t))  -  m(w_T^t) / (beta + Tb(w_T^t))
 *   S(w_T^0) = 0,  S(w_T^(t+1)) = S(w_T^t) + term_t  (t < T - 1),   closing = sum_{t<T} term_t.
 * The call creates a new ONE-ROW set of the same worker and length holding S's coefficients, exactly as if S's T evaluations
 * had gone through kzg_rows_commit(i, 1, S, T, 1, ..): out_commitment48 equals that call's byte for byte and *out_handle opens,
 * evaluates, combines, releases, goes stale and counts against KZG_MAX_ROW_SETS (KZG_E_BUSY; KZG_E_NOMEM on a failed
 * allocation) like any other.  out_closing32 is canonical big-endian: 0 exactly when the sum closes (every looked-up tuple is
 * in the table with the stated multiplicities, except with probability ~ (L + 1) T / r over beta).  The library does not judge
 * it.  Nothing row-sized crosses the host link in either direction.
 * Handle lists follow kzg_rows_open: 1 .. KZG_MAX_BATCH_OPEN handles each, a handle may repeat (also across the lists), unknown /
 * released / stale -> KZG_E_ARG; 1 <= w, 1 <= L, L * w <= KZG_MAX_BATCH_OPEN; the input concatenation must hold exactly L * w
 * rows, the table concatenation exactly w rows, the multiplicity set exactly one row; every set named must belong to one
 * worker and one (power-of-two) T; theta or beta >= r -> KZG_E_ARG.  A zero denominator (beta + F_l = 0 or beta + Tb = 0
 * somewhere on the domain) leaves S undefined: it is found on the device and answered with KZG_E_ARG and a message that says
 * so, no set created.  The source sets are only read; a release or an SRS load racing the call follows the rules of
 * kzg_rows_open.  Thread-safe like every call; after any error the context keeps serving.
 * SOUNDNESS: theta and beta must be drawn AFTER the commitments of the inputs, the table AND m are fixed (a prover who knows
 * them before it commits m can make a false lookup close).  The library derives no challenge and adds NO BLINDING (as for the
 * grand product).  closing = 0 is NOT the argument: the wrap-around relation S(w_T X) - S(X) = term(X) on all of H (which
 * forces closing = 0) belongs in the caller's quotient.
 * That quotient term (it needs S at X and w_T X, i.e. gate factors with a rotation) is the lookup part of
 * kzg_rows_commit_quotient_ext.
 * m itself is built and committed on the device by kzg_rows_commit_multiplicities.
 * Per-row selectors (a lookup enabled only on some rows): kzg_rows_commit_lookup_sum_sel below.  OUT OF SCOPE: plookup, a
 * selector on the table side.  Blinding rows: kzg_rows_commit_lookup_sum_zk below. */
int kzg_rows_commit_lookup_sum(kzg_ctx* ctx, uint32_t n_input_handles, const uint64_t* input_handles,
                               uint32_t n_table_handles, const uint64_t* table_handles, uint64_t mult_handle,
                               uint32_t n_lookups, uint32_t width, const uint8_t theta_be32[32], const uint8_t beta_be32[32],
                               uint8_t out_commitment48[48], uint8_t out_closing32[32], uint64_t* out_handle);
/* A fifth set built FROM sets: the multiplicity row m of the lookup argument above, computed and committed on the device from
 * rows that are already resident -- a hash join of the looked-up tuples against the table.  Handle lists, L = n_lookups,
 * w = width, the lookup-major input order, w_T and the natural order are those of kzg_rows_commit_lookup_sum.  Tuples are
 * compared as w-tuples of elements of Fr, in ALL w columns (no challenge exists yet: m is committed BEFORE theta and beta are
 * drawn, so the join is on the full tuples, never on a theta-compression):
 *   in(l, t) = (f_{l,0}(w_T^t), .., f_{l,w-1}(w_T^t)),    tab(t) = (t_0(w_T^t), .., t_{w-1}(w_T^t))
 *   first(u) = the smallest t with tab(t) = u
 *   m(w_T^t) = #{ (l, t') : first(in(l, t')) = t },       missing = #{ (l, t') : in(l, t') is no row of the table }
 * A tuple that occurs several times in the table gets ALL its hits on its first copy; the later copies get 0.  That makes m a
 * function of its inputs (the same bytes whatever the device's schedule).  (a, b) in the table does not make (b, a) a hit.
 * The call creates a new ONE-ROW set of the same worker and length holding m's coefficients, exactly as if m's T evaluations
 * had gone through kzg_rows_commit(i, 1, m, T, 1, ..): out_commitment48 equals that call's byte for byte and *out_handle opens,
 * evaluates, combines, releases, goes stale and counts against KZG_MAX_ROW_SETS (KZG_E_BUSY; KZG_E_NOMEM on a failed
 * allocation, the lane's workspace of 2 w T-element vectors included) like any other; it can be passed straight to
 * kzg_rows_commit_lookup_sum as mult_handle and named as mult_row in kzg_rows_commit_quotient_ext.  *out_missing is 0 exactly
 * when every looked-up tuple is in the table.  The library does not judge it, as it does not judge a closing value: the set is
 * created either way and m then counts only the cells that were found (the lookup sum over it does not close).  Nothing
 * row-sized crosses the host link in either direction.
 * Errors (all KZG_E_ARG unless said): handle lists as in kzg_rows_open (1 .. KZG_MAX_BATCH_OPEN handles each, a handle may
 * repeat, also across the lists; unknown / released / stale); w = 0, L = 0 or L * w > KZG_MAX_BATCH_OPEN; an input
 * concatenation that does not hold exactly L * w rows or a table concatenation that does not hold exactly w; sets of more
 * than one worker or row length; a row length that is no power of two or exceeds 2^27.  Every walk of the join is bounded by
 * the slot table's capacity; a walk that reaches the bound (it cannot, with 2 T slots for at most T tuples) is answered with
 * KZG_E_HIP and no set.  The source sets are only read; a release or an SRS load racing the call follows the rules of
 * kzg_rows_open.  Thread-safe like every call; after any error the context keeps serving.
 * SOUNDNESS: nothing here is a proof.  m is prover data like any witness row; the argument is the relation of
 * kzg_rows_commit_quotient_ext over S, with theta and beta drawn AFTER this call's commitment is fixed.  No blinding.
 * Per-row selectors: kzg_rows_commit_multiplicities_sel below.  OUT OF SCOPE: plookup, a selector on the table side (as
 * above).  Blinding rows: kzg_rows_commit_multiplicities_zk below. */
int kzg_rows_commit_multiplicities(kzg_ctx* ctx, uint32_t n_input_handles, const uint64_t* input_handles,
                                   uint32_t n_table_handles, const uint64_t* table_handles, uint32_t n_lookups, uint32_t width,
                                   uint8_t out_commitment48[48], uint64_t* out_missing, uint64_t* out_handle);
/* A third set built FROM sets: the PLONK quotient (round 3), computed and committed on the device from rows that are already
 * resident.  The concatenated rows of the handles (as in kzg_rows_open) are f_0 .. f_{n-1}, n <= KZG_MAX_BATCH_OPEN, all of
 * one worker and one power-of-two length T; everything below names a row by its index into that list.  A full standard PLONK
 * circuit is 13 rows: a b c | qL qR qO qM qC | sigma1 sigma2 sigma3 | z (and a public-input row where needed).
 *   Gate(X) = sum_u c_u prod_{j in term u} f_j(X)     gate->n_terms <= KZG_MAX_GATE_TERMS terms; term u has the canonical
 *             scalar c_u and term_lens[u] <= E + 1 row indices (term_rows holds the lists one after the other; an index may
 *             repeat; an empty list makes the constant term c_u).  Standard gate: [qL,a] [qR,b] [qO,c] [qM,a,b] [qC].
 *   P1(X)   = z(X) prod_j (a_j(X) + beta s_j X + gamma) - z(wX) prod_j (a_j(X) + beta sigma_j(X) + gamma),  j < perm->k
 *   P2(X)   = (z(X) - 1) L_0(X),   L_0(X) = (X^T - 1) / (T (X - 1))
 *   num     = Gate + alpha P1 + alpha^2 P2,   t = num / (X^T - 1)
 * with w the T-th root of unity of the grand product (7^((r-1)/T)).  perm == NULL or perm->k == 0 switches the permutation
 * part off (t = Gate / (X^T - 1); nothing else of perm is read).  E = 2^ext_log with ext_log in {1, 2, 3} is the factor by
 * which the work domain exceeds T; every term has at most E + 1 factors and perm->k <= E (P1 has k + 1), so deg num <
 * (E + 1) T and t has fewer than E T coefficients.  Standard PLONK: k = 3, ext_log = 2, n_pieces = 3 (deg t = 3T - 4).
 * The call creates a new set of n_pieces = P rows (1 <= P <= E) of the same worker and length: row p holds t's coefficients
 * [pT, (p+1)T), t = sum_p X^(pT) t_p.  out_commitments48[p] equals kzg_rows_commit(i, 1, t_p, T, evaluation_form = 0, ..)
 * byte for byte, and *out_handle opens, evaluates, combines, releases, goes stale and counts against KZG_MAX_ROW_SETS
 * (KZG_E_BUSY; KZG_E_NOMEM on a failed allocation, the lane's workspace of E T-element vectors included) like any other.
 * Nothing row-sized crosses the host link in either direction.
 * SHAPE CHECK: when P < E the device checks that every coefficient of t at index >= P T is zero; if one is not, the call
 * answers KZG_E_ARG with a message that says the constraints do not hold on the domain or P is too small, and creates no
 * set.  An unsatisfied row makes num / (X^T - 1) a non-polynomial whose interpolant on the work domain has full degree, so
 * broken instances are caught this way in practice -- but the check is a NECESSARY condition, NOT A PROOF that the
 * constraints hold: only the verifier's identity at a random point is.  When P = E nothing can be checked and nothing is.
 * Errors (all KZG_E_ARG unless said): handle rules as in kzg_rows_open (1 .. KZG_MAX_BATCH_OPEN handles, a handle may repeat,
 * unknown / released / stale); a row index >= n; more than E + 1 factors in a term; k > E; ext_log outside {1, 2, 3};
 * n_pieces outside [1, E]; more than KZG_MAX_GATE_TERMS terms; neither a term nor a permutation part; a scalar (c_u, s_j,
 * beta, gamma, alpha) >= r.  The source sets are only read; a release or an SRS load racing the call follows the rules of
 * kzg_rows_open.  Thread-safe like every call; after any error the context keeps serving.
 * SOUNDNESS: alpha must be drawn AFTER z's commitment is fixed, and beta, gamma after the wire commitments.  The library
 * derives no challenge and adds NO BLINDING here either: a blinded t or z has degree >= T per piece and does not fit T-point
 * slices; a caller who blinds pads its circuit below T and uses the blinding-rows layout of kzg_rows_commit_quotient_zk. */
#define KZG_MAX_GATE_TERMS 16
typedef struct kzg_quotient_gate {
    uint32_t n_terms;
    const uint8_t* coeffs_be32;  /* n_terms * 32 */
    const uint32_t* term_lens;   /* n_terms */
    const uint32_t* term_rows;   /* sum of term_lens */
} kzg_quotient_gate;
typedef struct kzg_quotient_perm {
    uint32_t k;
    uint32_t z_row;
    const uint32_t* wire_rows;   /* k */
    const uint32_t* sigma_rows;  /* k */
    const uint8_t* shifts_be32;  /* k * 32 */
    const uint8_t* beta_be32;    /* 32 */
    const uint8_t* gamma_be32;   /* 32 */
    const uint8_t* alpha_be32;   /* 32 */
} kzg_quotient_perm;
int kzg_rows_commit_quotient(kzg_ctx* ctx, uint32_t n_handles, const uint64_t* handles, const kzg_quotient_gate* gate,
                             const kzg_quotient_perm* perm /* NULL: gate only */, uint32_t ext_log, uint32_t n_pieces,
                             uint8_t* out_commitments48 /* n_pieces * 48 */, uint64_t* out_handle);
/* kzg_rows_commit_quotient with gate factors that may be ROTATED and with the logUp relation of kzg_rows_commit_lookup_sum as a
 * third part.  Everything not named here follows kzg_rows_commit_quotient: the handle rules, one worker and one power-of-two T,
 * E = 2^ext_log with ext_log in {1, 2, 3}, the pieces, the SHAPE CHECK when P < E (necessary, not a proof), the new set's life,
 * thread safety, "after any error the context keeps serving", no blinding, no derived challenge.  With every rotation 0 and
 * lookup == NULL the call IS kzg_rows_commit_quotient, byte for byte.
 *   Gate(X) = sum_u c_u prod_f f_{j(u,f)}(w^rot(u,f) X)    term_rots runs beside term_rows (NULL: every rotation 0): on the
 *             domain factor f reads row j at t + rot (mod T).  Any int32 rot is accepted and reduced mod T (-1 and T - 1, or
 *             1 and T + 1, give the same bytes).  A term still has at most E + 1 factors.  A rotated factor shares its row's
 *             extended vector with the unrotated one: no extra transform, no extra workspace.
 *   D_0     = beta + sum_c theta^c t_c,    D_l = beta + sum_c theta^c f_{l,c}  (l = 1 .. L)        (c < w; the rows f_{l,c} =
 *             input_rows[(l - 1) w + c], t_c = table_rows[c], m = mult_row, S = sum_row; theta, beta those S was built with)
 *   LK1(X)  = (S(wX) - S(X)) prod_{l=0..L} D_l  -  [ sum_{l=1..L} prod_{l' != l, l' = 0..L} D_l'  -  m prod_{l=1..L} D_l ]
 *   LK2(X)  = S(X) L_0(X)
 *   num     = Gate + alpha P1 + alpha^2 P2 + alpha^3 LK1 + alpha^4 LK2,   t = num / (X^T - 1)
 * The powers 3 and 4 of alpha are FIXED, whether or not a permutation part is present.  LK1 vanishes on all of H exactly when
 * the wrap-around relation S(wX) - S(X) = term(X) holds there, which forces closing = 0: this, not the closing value, is the
 * lookup argument.  LK1 has L + 2 factors, so L <= E - 1; the lookup part alone needs L + 1 pieces.  lookup == NULL: no
 * lookup part.  perm == NULL or perm->k == 0: no permutation part.
 * Errors beyond those of kzg_rows_commit_quotient (all KZG_E_ARG): L = 0, w = 0, L > E - 1 or L * w > KZG_MAX_BATCH_OPEN; a
 * lookup row index >= n; theta, beta or alpha >= r; lookup->alpha_be32 and perm->alpha_be32 (perm->k > 0) unequal in bytes;
 * no term, no permutation part and no lookup part; a null array inside a part that is present (gate itself must not be NULL;
 * n_terms = 0 makes it empty).
 * SOUNDNESS: alpha must be drawn AFTER the commitments of S and z are fixed; theta and beta AFTER the commitments of the
 * inputs, the table and m (as for kzg_rows_commit_lookup_sum; kzg_rows_commit_multiplicities builds and commits m on the
 * device).  Lookups enabled on some rows only: kzg_rows_commit_quotient_sel below.  Still out of scope: plookup, a selector
 * on the table side.  Blinding rows: kzg_rows_commit_quotient_zk below. */
typedef struct kzg_quotient_terms {
    uint32_t n_terms;
    const uint8_t* coeffs_be32;  /* n_terms * 32 */
    const uint32_t* term_lens;   /* n_terms */
    const uint32_t* term_rows;   /* sum of term_lens */
    const int32_t* term_rots;    /* sum of term_lens; NULL = every rotation 0 */
} kzg_quotient_terms;
typedef struct kzg_quotient_lookup {
    uint32_t n_lookups;          /* L */
    uint32_t width;              /* w */
    const uint32_t* input_rows;  /* L * w, lookup-major */
    const uint32_t* table_rows;  /* w */
    uint32_t mult_row;           /* m */
    uint32_t sum_row;            /* S */
    const uint8_t* theta_be32;   /* 32 */
    const uint8_t* beta_be32;    /* 32 */
    const uint8_t* alpha_be32;   /* 32 */
} kzg_quotient_lookup;
int kzg_rows_commit_quotient_ext(kzg_ctx* ctx, uint32_t n_handles, const uint64_t* handles, const kzg_quotient_terms* gate,
                                 const kzg_quotient_perm* perm /* NULL: none */,
                                 const kzg_quotient_lookup* lookup /* NULL: none */, uint32_t ext_log, uint32_t n_pieces,
                                 uint8_t* out_commitments48 /* n_pieces * 48 */, uint64_t* out_handle);
/* BLINDING ROWS: the four builders above for a circuit that hides its witness (the layout of halo2).  With T the row length
 * and u = usable, 1 <= u <= T - 1 and T - u <= KZG_MAX_BLIND_ROWS:
 *   rows 0 .. u - 1 carry the circuit; row u is the "last" row, where a running value closes; rows u + 1 .. T - 1 hold random
 *   values -- in the caller's own rows (wires, which it commits itself) and, for z, S and m, the T - u - 1 canonical scalars of
 *   tail_be32 (row u + 1 first; NULL exactly when u = T - 1).
 * The library draws no randomness, as it derives no challenge.  Everything not named here is that of the plain call: handle
 * rules, worker and T rules, the new set's life, thread safety, "after any error the context keeps serving"; nothing
 * row-sized crosses the host link (the tail rides in a kernel argument).  The plain calls keep their bytes, their kernels and
 * their host path.  Errors beyond the plain call's (all KZG_E_ARG): u = 0, u >= T, T - u > KZG_MAX_BLIND_ROWS, a tail scalar
 * >= r, tail_be32 NULL with u < T - 1.
 * kzg_rows_commit_grand_product_zk:  z(w^0) = 1,  z(w^(t+1)) = z(w^t) N_t / D_t for t < u, so z(w^u) = prod_{t<u} N_t / D_t =
 *   closing (1 when the permutation holds on the usable rows);  z(w^t) = tail[t - u - 1] for u < t < T.  Rows t >= u of the
 *   wires and sigmas do not enter the product: a zero D_t there is no error, one at t < u is the plain call's KZG_E_ARG.  The
 *   committed row equals kzg_rows_commit(i, 1, z, T, 1, ..) of those T evaluations byte for byte.  One inversion per call and
 *   the plain call's four-vector workspace.
 * kzg_rows_commit_lookup_sum_zk:  S(w_T^0) = 0,  S(w_T^(t+1)) = S(w_T^t) + term_t for t < u, S(w_T^u) = sum_{t<u} term_t =
 *   closing, the tail behind.  term_t is 0 for t >= u whatever the cells hold: a zero denominator there is no error.
 * kzg_rows_commit_multiplicities_zk:  only table rows t < u are built into the join and only input cells t' < u are probed;
 *   `missing` counts only those cells;  m(w_T^u) = 0 and m(w_T^t) = tail[t - u - 1] behind it.  The first-copy rule, the
 *   bounded walks and the overrun answer are the plain call's.
 * kzg_rows_commit_quotient_zk:  active names a resident row A, the caller's fixed column that is 1 on t < u and 0 elsewhere
 *   (the library does not judge its contents), which switches the two relations that run along the rows off behind u:
 *     num = Gate + alpha A P1 + alpha^2 P2 + alpha^3 A LK1 + alpha^4 LK2,   t = num / (X^T - 1)
 *   A P1 has k + 2 factors, so perm->k <= E - 1; A LK1 has L + 3, so L <= E - 2 (either violated: KZG_E_ARG; so is an
 *   active_row >= n).  With active == NULL the call IS kzg_rows_commit_quotient_ext, byte for byte.  What remains needs no
 *   library support: "z = 1 at row u" is (z - 1) L_u and "S = 0 at row u" is S L_u, ordinary gate terms over a caller row L_u
 *   (1 at row u, 0 elsewhere) with the caller's powers of alpha as coefficients; the gates themselves are switched off on the
 *   padding rows by the caller's selectors.
 * SOUNDNESS / HIDING: the library supplies the mechanics only.  How many blinding rows a polynomial needs (at least the number
 * of points it is opened at, plus one) is the caller's choice, and the random values must be fresh per proof.  The quotient
 * pieces are opened only through the combination sum_p zeta^(pT) t_p (kzg_rows_open_lincomb), whose value the identity already
 * fixes.  Challenges are still the caller's and are drawn as before (beta, gamma after the wires; theta, beta after the
 * inputs, the table and m; alpha after z and S).  Degree-raising blinders (b Z_H) do not fit a T-point slice and stay out of
 * scope, as do plookup and a selector on the table side.  Lookups enabled on some rows only: the _sel calls below (the
 * builders take usable and tail like the calls here, the quotient calls take the active column). */
#define KZG_MAX_BLIND_ROWS 32
typedef struct kzg_quotient_active {
    uint32_t active_row;         /* A */
} kzg_quotient_active;
int kzg_rows_commit_grand_product_zk(kzg_ctx* ctx, uint32_t n_wire_handles, const uint64_t* wire_handles,
                                     uint32_t n_sigma_handles, const uint64_t* sigma_handles, uint32_t k,
                                     const uint8_t* shifts_be32 /* k*32 */, const uint8_t beta_be32[32],
                                     const uint8_t gamma_be32[32], uint64_t usable,
                                     const uint8_t* tail_be32 /* (T-usable-1)*32, or NULL */, uint8_t out_commitment48[48],
                                     uint8_t out_closing32[32], uint64_t* out_handle);
int kzg_rows_commit_lookup_sum_zk(kzg_ctx* ctx, uint32_t n_input_handles, const uint64_t* input_handles,
                                  uint32_t n_table_handles, const uint64_t* table_handles, uint64_t mult_handle,
                                  uint32_t n_lookups, uint32_t width, const uint8_t theta_be32[32], const uint8_t beta_be32[32],
                                  uint64_t usable, const uint8_t* tail_be32 /* (T-usable-1)*32, or NULL */,
                                  uint8_t out_commitment48[48], uint8_t out_closing32[32], uint64_t* out_handle);
int kzg_rows_commit_multiplicities_zk(kzg_ctx* ctx, uint32_t n_input_handles, const uint64_t* input_handles,
                                      uint32_t n_table_handles, const uint64_t* table_handles, uint32_t n_lookups, uint32_t width,
                                      uint64_t usable, const uint8_t* tail_be32 /* (T-usable-1)*32, or NULL */,
                                      uint8_t out_commitment48[48], uint64_t* out_missing, uint64_t* out_handle);
int kzg_rows_commit_quotient_zk(kzg_ctx* ctx, uint32_t n_handles, const uint64_t* handles, const kzg_quotient_terms* gate,
                                const kzg_quotient_perm* perm /* NULL: none */,
                                const kzg_quotient_lookup* lookup /* NULL: none */,
                                const kzg_quotient_active* active /* NULL: kzg_rows_commit_quotient_ext */, uint32_t ext_log,
                                uint32_t n_pieces, uint8_t* out_commitments48 /* n_pieces * 48 */, uint64_t* out_handle);
/* LOOKUP SELECTORS: the multiplicities and the running sum for lookups that are enabled on some rows only (halo2's q * a).
 * A selector is an ordinary resident row of the same worker and length, the caller's fixed column q_l.  Each lookup l < L has
 * either one selector row or KZG_NO_SELECTOR (the constant 1); one row may serve several lookups.  sel_index[l] (L entries)
 * is KZG_NO_SELECTOR or indexes the concatenated rows of the sel_handles sets (at most KZG_MAX_BATCH_OPEN rows, handle rules of
 * kzg_rows_open), so a caller names its whole fixed set and picks the rows, without committing the selectors apart;
 * n_sel_handles = 0 (sel_handles may then be NULL) is legal only when every entry is KZG_NO_SELECTOR.  With q_l = 1 for a
 * lookup without a selector:
 *   m(w_T^t) = #{ (l, t') : q_l(w_T^t') != 0 and first(in(l, t')) = t },
 *   missing  = #{ (l, t') : q_l(w_T^t') != 0 and in(l, t') is no row of the table }
 *   term_t   = sum_l q_l(w_T^t) / (beta + F_l(w_T^t))  -  m(w_T^t) / (beta + Tb(w_T^t))
 * Multiplicities: cell (l, t) is probed exactly when q_l(w_T^t) != 0, compared as canonical words like the join's tuples; a
 * probed cell counts 1 whatever the value of q_l there, and `missing` counts probed cells only.  The table rows are all built as
 * before; the first-copy rule, the bounded walks and the overrun answer are unchanged.  Running sum: the fraction of lookup l
 * has the numerator q_l(w_T^t), ANY element of Fr -- per lookup the update is (P, Q) <- (P d + q Q, Q d) with d = beta + F_l.
 * From the two rules: m and S agree (the sum closes for a satisfied instance) exactly when q_l is 0 or 1 on the rows that
 * count; the library does not judge q, as it judges no closing value.  A zero denominator is still KZG_E_ARG wherever the
 * plain or _zk rule reads that row, whether the row is enabled or not (the quotient relation carries D_l on every row, and
 * beta is random).
 * Layout: usable and tail_be32 are those of the _zk calls (rows >= usable are neither probed nor summed, row usable closes,
 * the tail behind); in addition usable == T with tail_be32 == NULL is the plain layout without a closing row.  So there is
 * ONE _sel builder per stage.  With every entry KZG_NO_SELECTOR each call IS the existing one byte for byte and kernel for
 * kernel (kzg_rows_commit_multiplicities / _lookup_sum for usable == T, their _zk forms otherwise); an all-ones selector row
 * gives the same bytes; selectors that are 0 everywhere give m = 0 on the circuit rows, missing = 0, S = 0 and closing 0.
 * Cost: each DISTINCT selector row is brought to evaluation form once per call (one forward transform and one more T-element
 * vector of lane workspace, counted in the KZG_E_NOMEM path); a selected lookup's probe reads 32 bytes more per cell and its
 * step of the running fraction does one product more.  Lookups without a selector launch the existing kernels.
 * Errors beyond the underlying call's (all KZG_E_ARG): sel_index NULL; sel_handles NULL with n_sel_handles > 0; more than
 * KZG_MAX_BATCH_OPEN selector handles or rows; an entry that is neither KZG_NO_SELECTOR nor below the number of selector rows
 * (so any real index with n_sel_handles = 0); a selector set of another worker or row length, or an unknown / released /
 * stale one.  Everything else -- thread safety, a racing release or SRS load, "after any error the context keeps serving" --
 * is the underlying call's.
 * The quotient calls are declared behind kzg_rows_quotient_part below (THE QUOTIENT WITH LOOKUP SELECTORS). */
#define KZG_NO_SELECTOR 0xffffffffu
int kzg_rows_commit_multiplicities_sel(kzg_ctx* ctx, uint32_t n_input_handles, const uint64_t* input_handles,
                                       uint32_t n_table_handles, const uint64_t* table_handles, uint32_t n_sel_handles,
                                       const uint64_t* sel_handles, const uint32_t* sel_index /* n_lookups */,
                                       uint32_t n_lookups, uint32_t width, uint64_t usable,
                                       const uint8_t* tail_be32 /* (T-usable-1)*32, or NULL */, uint8_t out_commitment48[48],
                                       uint64_t* out_missing, uint64_t* out_handle);
int kzg_rows_commit_lookup_sum_sel(kzg_ctx* ctx, uint32_t n_input_handles, const uint64_t* input_handles,
                                   uint32_t n_table_handles, const uint64_t* table_handles, uint64_t mult_handle,
                                   uint32_t n_sel_handles, const uint64_t* sel_handles,
                                   const uint32_t* sel_index /* n_lookups */, uint32_t n_lookups, uint32_t width,
                                   const uint8_t theta_be32[32], const uint8_t beta_be32[32], uint64_t usable,
                                   const uint8_t* tail_be32 /* (T-usable-1)*32, or NULL */, uint8_t out_commitment48[48],
                                   uint8_t out_closing32[32], uint64_t* out_handle);
/* THE QUOTIENT IN PARTS, AND CHAINED GRAND PRODUCTS: circuits that fit no single quotient call -- more than 16 rows, more
 * permuted columns than E (E - 1 with an active column), several permutation or lookup arguments, more than 16 gate terms.
 * The quotient is linear in its numerator and the division by X^T - 1 is pointwise on the coset g H_N, so the numerator is
 * summed on the device over several calls, each under the caps above with its own handles and its own row numbering (halo2's
 * layout: the permutation split into chunks of E - 1 columns with one z_c each, chained by z_c(1) = z_{c-1}(w^u)).
 * kzg_rows_quotient_part:  computes this part's num_p / Z_H on the coset exactly as kzg_rows_commit_quotient_zk does (handle
 *   rules, row numbering, the degree rules per part and the scalar checks are that call's; active == NULL and lookup == NULL
 *   as there), multiplies it by the canonical scalar scale (NULL: 1) and adds it into the accumulator *inout_acc, a device
 *   vector of N = E T canonical elements.  *inout_acc == 0 creates the accumulator (the part is written, not added) and
 *   returns its handle there.  The caller keeps parts apart with its own powers of alpha in scale: inside a part, alpha still
 *   weighs P1, P2, LK1, LK2 as in the single call.
 *   link != NULL (needs perm->k > 0, else KZG_E_ARG): P2 is (z(X) - f_prev(w^rot X)) L_0(X) instead of (z(X) - 1) L_0(X), with
 *   f_prev row prev_row of THIS part's concatenation and rot any int32, reduced mod T like a gate rotation and read from the
 *   same extended vector at index (i + rot E) mod N -- the chain relation z_c(1) = z_{c-1}(w^u) with rot = u.  The last chunk's
 *   closing relation (z - 1) L_u stays a gate term over the caller's row L_u, as in the single call.
 * The accumulator is an entry of the set table, not a row set: its handle comes from the same counter, it counts against
 *   KZG_MAX_ROW_SETS and in kzg_rows_stats (N * 32 bytes), goes stale on an SRS load, is freed by kzg_rows_release and
 *   kzg_destroy, and its buffer goes through the same free list.  It remembers the worker, T and ext_log of its first part; a
 *   part that differs in any of them gets KZG_E_ARG.  Naming it in an open, an evaluation, a lincomb or any builder is
 *   KZG_E_ARG, and so is naming a row set as the accumulator.  Parts added to one accumulator from several threads are
 *   serialised by the library at the add (the rest of each part overlaps); field addition is exact, so the order changes no byte.
 *   An error never changes which handles are live: a failed first part creates nothing; a failed later part leaves the
 *   accumulator as it was (the add is the call's last device step); if the add itself fails with KZG_E_HIP the accumulator
 *   becomes stale.
 * kzg_rows_quotient_finish:  the inverse transform, the pieces with the shape check when n_pieces < E, and the one MSM pass --
 *   the code of the single call.  On KZG_OK the new set of n_pieces rows exists and the accumulator is consumed (its handle is
 *   dead).  On ANY error, the shape check's KZG_E_ARG included, no set is created and the accumulator stays live for the caller
 *   to release.  n_pieces outside [1, E], a row-set handle, a released or stale accumulator: KZG_E_ARG.
 * One part with scale NULL and no link followed by finish equals the single call byte for byte.
 * kzg_rows_commit_grand_product_chain:  kzg_rows_commit_grand_product_zk with start_be32 in front of the outputs:
 *   z(w^0) = start, z(w^(t+1)) = z(w^t) N_t / D_t for t < u, so z(w^u) = start * prod N / prod D, returned as closing; the tail
 *   sits behind it untouched by start.  start >= r or start = 0: KZG_E_ARG.  start = 1 IS the _zk call byte for byte.  The factor
 *   is folded in at the scan's top level: no pass over T elements.  Only the blinding-rows layout has a row that holds the
 *   closing value, so there is no plain form.
 * COST: each part re-extends the rows it names -- a row shared by two parts is transformed twice; that is the price of the caps
 *   staying where they are.  Workspace per part is the single call's; the accumulator adds N * 32 bytes.
 * SOUNDNESS: the library supplies the mechanics only.  The scales (and every alpha inside a part) must be drawn after all
 *   z_c and S are committed; the chunks' z_c must share beta and gamma; the verifier recomputes sum_p scale_p num_p(zeta) from
 *   the opened values, the link as (z_c(zeta) - z_{c-1}(w^u zeta)) L_0(zeta).
 * OUT OF SCOPE: an opening over more than 16 rows (a wide circuit opens in several kzg_rows_open_lincomb calls, one proof per
 *   call and point); sharing extended rows between parts; plookup; degree-raising blinders; deriving challenges or scales
 *   (the library still draws nothing).  Lookup selectors in a part: kzg_rows_quotient_part_sel below. */
typedef struct kzg_quotient_link {
    uint32_t prev_row;           /* f_prev: the previous chunk's z */
    int32_t rot;                 /* read at w^rot X */
} kzg_quotient_link;
int kzg_rows_quotient_part(kzg_ctx* ctx, uint32_t n_handles, const uint64_t* handles, const kzg_quotient_terms* gate,
                           const kzg_quotient_perm* perm /* NULL: none */, const kzg_quotient_link* link /* NULL: P2 = (z - 1) L_0 */,
                           const kzg_quotient_lookup* lookup /* NULL: none */, const kzg_quotient_active* active /* NULL: none */,
                           uint32_t ext_log, const uint8_t* scale_be32 /* NULL: 1 */, uint64_t* inout_acc /* 0: create */);
int kzg_rows_quotient_finish(kzg_ctx* ctx, uint64_t acc, uint32_t n_pieces, uint8_t* out_commitments48 /* n_pieces * 48 */,
                             uint64_t* out_handle);
int kzg_rows_commit_grand_product_chain(kzg_ctx* ctx, uint32_t n_wire_handles, const uint64_t* wire_handles,
                                        uint32_t n_sigma_handles, const uint64_t* sigma_handles, uint32_t k,
                                        const uint8_t* shifts_be32 /* k*32 */, const uint8_t beta_be32[32],
                                        const uint8_t gamma_be32[32], uint64_t usable,
                                        const uint8_t* tail_be32 /* (T-usable-1)*32, or NULL */, const uint8_t start_be32[32],
                                        uint8_t out_commitment48[48], uint8_t out_closing32[32], uint64_t* out_handle);
/* THE SHUFFLE: a set built FROM sets, the running product of a shuffle argument ("the tuples of these columns are, as a
 * multiset over the rows, the tuples of those columns": memory consistency, sorted-column range checks, data handed between
 * regions), computed and committed on the device from rows that are already resident.  It has no table and no
 * multiplicities.  The concatenated rows of the input_handles sets are the G * w rows a_{g,c}, group-major (g < G = n_groups,
 * c < w = width, the order of the lookups' inputs); those of the shuffle_handles sets are the G * w rows b_{g,c}.  With w_T
 * the T-th root of unity of evaluation_form = 1 rows (7^((r-1)/T), natural order) and t in [0, T):
 *   A_g(w_T^t) = sum_c theta^c a_{g,c}(w_T^t),   B_g(w_T^t) = sum_c theta^c b_{g,c}(w_T^t)       (theta unused when w = 1)
 *   nf_g = gamma + A_g                    df_g = gamma + B_g                    (no selector on that side of group g)
 *   nf_g = 1 + q_g (gamma + A_g - 1)      df_g = 1 + q'_g (gamma + B_g - 1)     (with a selector row q_g / q'_g)
 *   N_t = prod_g nf_g(w_T^t),   D_t = prod_g df_g(w_T^t)
 *   z(w_T^0) = 1,  z(w_T^(t+1)) = z(w_T^t) N_t / D_t  (t < T - 1),   closing = prod_t N_t / prod_t D_t.
 * The call creates a new ONE-ROW set of the same worker and length holding z's coefficients, exactly as if z's T evaluations
 * had gone through kzg_rows_commit(i, 1, z, T, 1, ..): out_commitment48 equals that call's byte for byte and *out_handle opens,
 * evaluates, combines, releases, goes stale and counts against KZG_MAX_ROW_SETS (KZG_E_BUSY; KZG_E_NOMEM on a failed
 * allocation -- the lane's workspace is the grand product's four T-element vectors and scan scratch plus ONE more T-element
 * vector when a selector is named, whatever G and w are) like any other.  out_closing32 is canonical big-endian: 1 exactly
 * when the product closes.  The library does not judge it.  Nothing row-sized crosses the host link in either direction (the
 * tail rides in a kernel argument).
 * opts (NULL: no selectors, plain layout):
 *   Selectors are ordinary resident rows of the same worker and length, the caller's fixed columns, addressed as in the _sel
 *   calls: input_sel[g] / shuffle_sel[g] (G entries each; a NULL list: none on that side) is KZG_NO_SELECTOR or indexes the
 *   concatenated rows of the sel_handles sets; one row may serve several places.  A disabled cell (q = 0) contributes the
 *   factor 1 whatever it holds; with boolean selectors the product closes exactly when the enabled input tuples are a
 *   permutation of the enabled shuffle tuples.  The library does not judge a selector's contents, as it does not judge the
 *   active column; an all-ones selector row gives the bytes of the call without it.
 *   usable = 0 is the plain layout.  Anything else is the layout of kzg_rows_commit_grand_product_zk with u = usable:
 *   N_t = D_t = 1 on the rows t >= u (a zero df there is no error), z(w_T^u) = closing, z(w_T^t) = tail[t - u - 1] behind it;
 *   1 <= u <= T - 1, T - u <= KZG_MAX_BLIND_ROWS, tail_be32 NULL exactly when u = T - 1.
 *   With opts == NULL, or usable == 0 and every entry KZG_NO_SELECTOR, exactly the plain path runs.
 * Handle lists follow kzg_rows_open: 1 .. KZG_MAX_BATCH_OPEN handles each, a handle may repeat (also across the lists), unknown /
 * released / stale -> KZG_E_ARG; every set named must belong to one worker and one (power-of-two) T.  KZG_E_ARG with a message
 * that names the cause: G = 0, w = 0 or G * w > KZG_MAX_BATCH_OPEN; an input or shuffle concatenation that does not hold
 * exactly G * w rows; a selector index that is neither KZG_NO_SELECTOR nor below the number of selector rows; selector indices
 * given with no selector handles; theta, gamma or a tail scalar >= r; u >= T, T - u > KZG_MAX_BLIND_ROWS, tail_be32 NULL with
 * u < T - 1, or a tail with usable = 0.  A zero denominator (some D_t = 0 on a row that counts) leaves z undefined: it is found
 * on the device and answered with KZG_E_ARG "zero denominator", no set created.  The source sets are only read; a release or an
 * SRS load racing the call follows the rules of kzg_rows_open.  Thread-safe like every call; after any error the context keeps
 * serving.
 * SOUNDNESS: theta and gamma must be drawn AFTER the commitments of all input and shuffle rows are fixed.  closing = 1 is NOT
 * the argument: the relation z(w_T X) prod_g df_g(X) = z(X) prod_g nf_g(X) on the rows that count belongs in the caller's
 * quotient, where it is a sum of products of rows at rotations 0 and 1 -- gate terms of kzg_rows_commit_quotient_ext / _zk /
 * kzg_rows_quotient_part, no new quotient call.  "z = 1 at row 0" and, under blinding, "z = 1 at row u" stay ordinary gate terms
 * over a caller row L_0 / L_u, as for the permutation.  There is NO BLINDING beyond the rows the caller passes, and the library
 * derives no challenge. */
typedef struct kzg_shuffle_opts {
    uint32_t n_sel_handles;
    const uint64_t* sel_handles;
    const uint32_t* input_sel;     /* G entries, KZG_NO_SELECTOR = none; NULL = none at all */
    const uint32_t* shuffle_sel;   /* the same for the shuffle side */
    uint64_t usable;               /* 0: plain layout; else the _zk layout */
    const uint8_t* tail_be32;      /* (T - usable - 1) * 32, or NULL */
} kzg_shuffle_opts;
int kzg_rows_commit_shuffle(kzg_ctx* ctx, uint32_t n_input_handles, const uint64_t* input_handles,
                            uint32_t n_shuffle_handles, const uint64_t* shuffle_handles, uint32_t n_groups, uint32_t width,
                            const uint8_t theta_be32[32], const uint8_t gamma_be32[32],
                            const kzg_shuffle_opts* opts /* NULL: no selectors, plain layout */, uint8_t out_commitment48[48],
                            uint8_t out_closing32[32], uint64_t* out_handle);
/* THE SORTED COLUMNS: a set built FROM sets, the second side of a shuffle whose first side is a group of columns and whose second
 * side is the same tuples SORTED (memory consistency: (addr, time | value) ordered by address then time; sorted-column range
 * checks), sorted and committed on the device from rows that are already resident.  The concatenated rows of the input_handles
 * sets are the w = width columns c_0 .. c_{w-1}, 1 <= w <= KZG_MAX_BATCH_OPEN.  With w_T the T-th root of unity of
 * evaluation_form = 1 rows (natural order), row t carries the tuple u_t = (c_0(w_T^t), .., c_{w-1}(w_T^t)).  Every entry is taken
 * as its CANONICAL INTEGER in [0, r) -- not as its Montgomery representative, whose words do not order like the values.  The
 * call creates a new set of w rows of the same worker and length whose evaluations are the tuples of rows [0, n), STABLY sorted:
 * ascending, lexicographic on the first n_keys columns (1 <= n_keys <= w), column 0 most significant, ties by ascending source
 * row t; the columns behind the keys travel with their row as payload.  The output is a function of the input bytes alone,
 * whatever the device's schedule.  out_commitments48[c] equals kzg_rows_commit(i, w, sorted rows, T, 1, ..)[c] byte for byte,
 * and *out_handle opens, evaluates, combines, releases, goes stale and counts against KZG_MAX_ROW_SETS (KZG_E_BUSY; KZG_E_NOMEM
 * on a failed allocation, the lane's workspace included: w + n_keys + 1 T-element vectors and about a third of one more for the
 * permutations and counts) like any other.
 * opts (NULL: plain layout):
 *   usable = 0 is the plain layout: n = T, all rows are sorted, tail_be32 must be NULL.  Otherwise n = usable, 1 <= usable <=
 *   T - 1 and T - usable <= KZG_MAX_BLIND_ROWS: source rows t >= usable are never read into the sort (they may hold anything),
 *   and output row usable + s of column c takes tail_be32[c * (T - usable) + s], column-major canonical scalars.  Unlike the
 *   _zk builders there is NO closing row: all T - usable rows behind are the caller's.  The tail (at most 16 KB) rides in kernel
 *   arguments; nothing row-sized crosses the host link in either direction.
 * The cost follows the significant bytes of the keys, not 255 bits: a key byte that is the same in all n rows costs nothing
 * (a column of 16-bit values costs 2 radix passes of the 32 a full-width column costs).
 * Handle lists follow kzg_rows_open: 1 .. KZG_MAX_BATCH_OPEN handles, a handle may repeat (two equal columns), unknown /
 * released / stale -> KZG_E_ARG; every set named must belong to one worker and one (power-of-two) T.  KZG_E_ARG with a message
 * that names the cause: w = 0 or w > KZG_MAX_BATCH_OPEN; n_keys = 0 or n_keys > w; a concatenation that does not hold exactly w
 * rows; T > 2^27; usable >= T; T - usable > KZG_MAX_BLIND_ROWS; a tail with usable = 0, or none with usable > 0; a tail scalar
 * >= r.  The source sets are only read; a release or an SRS load racing the call follows the rules of kzg_rows_open.
 * Thread-safe like every call; after any error the context keeps serving.
 * OUT OF SCOPE: selectors (the caller compacts the enabled rows itself) and descending order.  (The permutation and its
 * inverse: carry the row number as a payload column, then kzg_rows_commit_fetch below by it.)
 * SOUNDNESS: nothing here is a proof.  The sorted rows are prover data; the argument is the shuffle relation
 * (kzg_rows_commit_shuffle over the inputs and this set, theta and gamma drawn AFTER these commitments are fixed) plus the
 * caller's adjacent-row gate.  The library derives no challenge. */
typedef struct kzg_sorted_opts {
    uint64_t usable;           /* 0: plain layout (all T rows are sorted); else only rows [0, usable) */
    const uint8_t* tail_be32;  /* width * (T - usable) * 32, column-major; NULL exactly when usable == 0 */
} kzg_sorted_opts;
int kzg_rows_commit_sorted(kzg_ctx* ctx, uint32_t n_input_handles, const uint64_t* input_handles,
                           uint32_t width, uint32_t n_keys, const kzg_sorted_opts* opts /* NULL: plain */,
                           uint8_t* out_commitments48 /* width * 48 */, uint64_t* out_handle);
/* THE DERIVED COLUMNS: a set built FROM sets, the two helper columns of range checks and zero tests, each a pure function of ONE
 * column that is already resident.  The concatenated rows of the input_handles sets (as in kzg_rows_open) are the source
 * columns; with w_T the T-th root of unity of evaluation_form = 1 rows, cell t of a column is its value at w_T^t, taken as its
 * CANONICAL INTEGER x_t in [0, r) -- not as its Montgomery representative.  Each of the n_ops ops names one source row and
 * yields `count` output rows; the outputs follow the order of ops, and inside one op the order given here:
 *   KZG_DERIVE_INV0 (bits = 0; count 1 or 2): inv0_t = x_t^-1 in the field, or 0 where x_t = 0 (the IsZero / "a != b" gadget);
 *     with count = 2 a second row follows, 1 where x_t = 0 and 0 elsewhere (the bit 1 - x inv0).  out_counts[op] is the number
 *     of zero cells among the rows read.  A zero is never an error.  All INV0 ops of one call share ONE batched inversion
 *     over n_inv * T elements: one field inversion per call, three to four products per cell.
 *   KZG_DERIVE_LIMBS (bits = b in [1, 32]; count = L in [1, KZG_MAX_BATCH_OPEN], b * L <= 256): limb_l,t = (x_t >> (b l)) & (2^b - 1)
 *     for l < L, least significant first: the rows a 2^b-entry table is looked up with (kzg_rows_commit_multiplicities ->
 *     kzg_rows_commit_lookup_sum) and the gate x = sum_l 2^(b l) limb_l ties back to x (kzg_rows_commit_quotient).
 *     out_counts[op] is the number of cells read with x_t >= 2^(b L) -- the part `missing` plays in the multiplicities call;
 *     the low limbs are still written for such cells and the call still succeeds.
 * n_out = sum of the counts, 1 <= n_out <= KZG_MAX_BATCH_OPEN.  The call creates a new set of n_out rows of the same worker and
 * length.  out_commitments48[c] equals kzg_rows_commit(i, n_out, derived rows, T, 1, ..)[c] byte for byte, and *out_handle
 * opens, evaluates, combines, releases, goes stale and counts against KZG_MAX_ROW_SETS (KZG_E_BUSY; KZG_E_NOMEM on a failed
 * allocation, the lane's workspace included: one T-element vector per DISTINCT source row, which is transformed once however
 * many ops name it, one per INV0 op, and max(number of INV0 ops, largest count) more) like any other.
 * opts (NULL: plain layout) follows kzg_sorted_opts:
 *   usable = 0 is the plain layout: all T rows are read, tail_be32 must be NULL.  Otherwise 1 <= usable <= T - 1 and T - usable
 *   <= KZG_MAX_BLIND_ROWS: source rows t >= usable are never read or counted (they may hold anything), and output row usable + s
 *   of output column c takes tail_be32[c * (T - usable) + s], column-major canonical scalars over the n_out columns.  There is
 *   NO closing row.  The tail rides in kernel arguments; nothing row-sized crosses the host link in either direction.
 * Handle lists follow kzg_rows_open: 1 .. KZG_MAX_BATCH_OPEN handles, a handle may repeat, unknown / released / stale ->
 * KZG_E_ARG; every set named must belong to one worker and one (power-of-two) T.  KZG_E_ARG with a message that begins
 * "derived:" and names the cause: n_ops = 0; n_out = 0 or n_out > KZG_MAX_BATCH_OPEN; an unknown kind; a row at or beyond the
 * concatenation; bits outside [1, 32], count outside [1, KZG_MAX_BATCH_OPEN] or b * L > 256 on LIMBS; bits != 0 or count
 * outside {1, 2} on INV0; usable >= T; T - usable > KZG_MAX_BLIND_ROWS; a tail with usable = 0, or none with usable > 0; a tail
 * scalar >= r.  The source sets are only read; a release or an SRS load racing the call follows the rules of kzg_rows_open.
 * Thread-safe like every call; after any error the context keeps serving.
 * OUT OF SCOPE: per-row selectors; signed limbs or limbs in a base that is no power of two.  (halo2's running-sum decomposition
 * along the rows: kzg_rows_commit_recurrence below, z' = (z - k) 2^-K as a recurrence.  General expression rows, sum_u c_u prod
 * rows[rot] committed as a column: kzg_rows_commit_expr below.  Machine-word arithmetic on the canonical integers -- bitwise
 * ops, carries, borrows, high products, quotients and remainders, shifts: kzg_rows_commit_int below.)
 * SOUNDNESS: nothing here is a proof.  The derived rows are prover data; the argument is the caller's gates (x inv0 = 1 - bit
 * and x bit = 0; x = sum_l 2^(b l) limb_l) and the lookup of the limbs, with every challenge drawn AFTER these commitments are
 * fixed.  The library derives no challenge and draws no randomness: the tail must be fresh per proof. */
#define KZG_DERIVE_INV0  1
#define KZG_DERIVE_LIMBS 2
typedef struct kzg_derive_op {
    uint32_t kind;   /* KZG_DERIVE_* */
    uint32_t row;    /* source row, index into the concatenated rows of input_handles */
    uint32_t bits;   /* LIMBS: b in [1, 32]; INV0: must be 0 */
    uint32_t count;  /* output rows of this op -- INV0: 1 (inv0) or 2 (inv0, then the is-zero bit);
                        LIMBS: L in [1, KZG_MAX_BATCH_OPEN], b * L <= 256 */
} kzg_derive_op;
typedef struct kzg_derive_opts {
    uint64_t usable;           /* 0: plain layout (all T rows are read); else only rows [0, usable) */
    const uint8_t* tail_be32;  /* n_out * (T - usable) * 32, column-major; NULL exactly when usable == 0 */
} kzg_derive_opts;
int kzg_rows_commit_derived(kzg_ctx* ctx, uint32_t n_input_handles, const uint64_t* input_handles,
                            uint32_t n_ops, const kzg_derive_op* ops, const kzg_derive_opts* opts /* NULL: plain */,
                            uint8_t* out_commitments48 /* n_out * 48 */, uint64_t* out_counts /* n_ops */,
                            uint64_t* out_handle);
/* THE EXPRESSION COLUMNS: a set built FROM sets, every output column plain arithmetic in columns that are already resident --
 * c = a b + q d, a theta-compressed tuple, the next row of a running value, the left side of any custom gate.  The concatenated
 * rows of the input_handles sets (as in kzg_rows_commit_derived) are the source columns; cell t of a column is its value at
 * w_T^t.  Expression e is a list of terms in the format of kzg_rows_commit_quotient_ext's gate (kzg_quotient_terms), evaluated on
 * H itself, not on the extended coset: for every row t < n, with n = usable, or n = T in the plain layout,
 *   v_e[t] = sum_u c_u prod_f col_{j(u,f)}[(t + rot(u,f)) mod T]
 * with 1 <= n_terms <= KZG_MAX_GATE_TERMS terms of 0 .. KZG_MAX_EXPR_FACTORS factors each; a term with no factors is the
 * constant c_u.  term_rots runs beside term_rows (NULL: every rotation 0); any int32 rotation is accepted and reduced mod T (-1
 * and T - 1, or 0 and T, give the same bytes).  A rotated factor of a row t < n reads the source cell it lands on, even at or
 * behind `usable`, as the quotient does; no source cell is read on behalf of a row t >= n.
 * flags = 0: the expression is COMMITTED.  The n_out committed expressions become, in their order, the rows of ONE new set of
 * the same worker and length; out_commitments48[c] equals kzg_rows_commit(i, n_out, the T evaluations, T, 1, ..)[c] byte for
 * byte, and *out_handle opens, evaluates, combines, releases, goes stale and counts against KZG_MAX_ROW_SETS (KZG_E_BUSY;
 * KZG_E_NOMEM on a failed allocation, the lane's workspace included: one T-element vector per DISTINCT source row that some
 * term names -- transformed once however many factors name it; a row no term names is not transformed -- and one more) like
 * any other.  flags = KZG_EXPR_CHECK: the expression is evaluated and counted only -- no row, no commitment: a device-side
 * "mock prover" for a gate, which the quotient would refuse only after all its work and without a row index.
 * out_nonzero[e] is the number of rows t < n with v_e[t] != 0 and out_first[e] the smallest such t, or KZG_EXPR_NONE; both are
 * filled for EVERY expression, committed or not.  If every expression is a check (n_out = 0) the call creates no set:
 * *out_handle = 0, out_commitments48 may be NULL, no reservation is made, nothing counts against KZG_MAX_ROW_SETS, and neither
 * an inverse transform nor an MSM runs.
 * opts (NULL: plain layout) is kzg_derive_opts in layout and refusals: usable = 0 is the plain layout, tail_be32 must be NULL.
 * Otherwise 1 <= usable <= T - 1, T - usable <= KZG_MAX_BLIND_ROWS, and output row usable + s of committed column c takes
 * tail_be32[c * (T - usable) + s], column-major canonical scalars over the n_out COMMITTED columns (with n_out = 0 the tail is
 * empty: tail_be32 is not read and may be NULL).  There is NO closing row.
 * Handle rules, the worker and T rules, the life of the new set, thread safety and "after any error the context keeps
 * serving" are those of kzg_rows_commit_derived.  KZG_E_ARG with a message that begins "expr:" and names the cause: n_exprs
 * outside [1, KZG_MAX_BATCH_OPEN]; n_terms outside [1, KZG_MAX_GATE_TERMS]; a term of more than KZG_MAX_EXPR_FACTORS factors;
 * flags other than 0 or KZG_EXPR_CHECK; a row index at or beyond the concatenation; a coefficient >= r (checked on the HOST,
 * before any lane is taken: an argument error, not a queued failure); a NULL array inside an expression (coeffs_be32,
 * term_lens, or term_rows when some term has a factor); T > 2^32 (the prepared rotations are 32-bit words); and the usable and
 * tail refusals of kzg_rows_commit_derived.
 * OUT OF SCOPE: division or an inverse inside an expression (compose with KZG_DERIVE_INV0); per-row selectors other than as an
 * ordinary factor; more than KZG_MAX_GATE_TERMS terms (split the expression and add the parts with a further call).  (The
 * running-sum decomposition along the rows, row t + 1 of the OUTPUT depending on row t of the output: kzg_rows_commit_recurrence
 * below.)
 * SOUNDNESS: nothing here is a proof.  An expression column is prover data: the argument is the caller's gate in the quotient
 * (kzg_rows_commit_quotient*), with every challenge that enters a coefficient drawn after the commitments it depends on are
 * fixed.  A zero count of a check is a convenience for the prover -- it tells where a witness is wrong before the quotient
 * is paid -- and convinces no verifier.  The library derives no challenge and draws no randomness: the tail must be fresh
 * per proof. */
#define KZG_MAX_EXPR_FACTORS 8
#define KZG_EXPR_CHECK 1u                   /* flags: evaluate and count only; no row, no commitment */
#define KZG_EXPR_NONE  0xffffffffffffffffull
typedef struct kzg_expr {
    kzg_quotient_terms terms;               /* coeffs_be32, term_lens, term_rows, term_rots (NULL: all 0) */
    uint32_t flags;                         /* 0 or KZG_EXPR_CHECK */
} kzg_expr;
typedef struct kzg_expr_opts {
    uint64_t usable;           /* 0: plain layout (all T rows are evaluated); else only rows [0, usable) */
    const uint8_t* tail_be32;  /* n_out * (T - usable) * 32, column-major; NULL when usable == 0 (and, if wished, when n_out == 0) */
} kzg_expr_opts;
int kzg_rows_commit_expr(kzg_ctx* ctx, uint32_t n_input_handles, const uint64_t* input_handles,
                         uint32_t n_exprs, const kzg_expr* exprs, const kzg_expr_opts* opts /* NULL: plain */,
                         uint8_t* out_commitments48 /* n_out * 48 */, uint64_t* out_nonzero /* n_exprs */,
                         uint64_t* out_first /* n_exprs */, uint64_t* out_handle);
/* THE RECURRENCE COLUMNS: a set built FROM sets, every output column a running value along the rows whose step is plain
 * arithmetic in columns that are already resident -- the running-sum range decomposition z' = (z - k) 2^-K, a random-linear-
 * combination or Horner accumulator acc' = acc r + byte, a running count or sum, a custom running product, and, where a selector
 * makes the multiplier 0, any of these restarted per segment.  The concatenated rows of the input_handles sets are the source
 * columns, with the handle, worker and T rules of kzg_rows_commit_expr.  Recurrence e has a multiplier expression mul, an addend
 * expression add and a start; mul and add are kzg_quotient_terms in exactly the format and with the caps of an expression of
 * kzg_rows_commit_expr (at most KZG_MAX_GATE_TERMS terms of at most KZG_MAX_EXPR_FACTORS factors, term_rots NULL: every
 * rotation 0), except that n_terms = 0 is allowed: an empty mul is A = 1, an empty add is B = 0; both empty is refused.  With
 * n = T in the plain layout and n = usable otherwise,
 *   v[0] = start,   v[t + 1] = A[t] v[t] + B[t]   for 0 <= t < n,
 * A[t] and B[t] the values of the two expressions at row t as kzg_rows_commit_expr defines them: a rotated factor reads the
 * source cell it lands on, also at or behind `usable`; nothing is read on behalf of a row t >= n.  A zero multiplier is never
 * an error: the value restarts at the addend.  Any start below r is legal, 0 included.
 * PLAIN LAYOUT (opts NULL, or usable = 0; tail_be32 must be NULL): rows 0 .. T - 1 hold v[0] .. v[T - 1]; out_closings32[e] is
 * v[T], the wrap-around value, 32 big-endian bytes.  It equals start exactly when the cyclic relation v(w X) = A v + B holds on
 * all of H.
 * USABLE LAYOUT (that of the _zk builders, not of kzg_rows_commit_derived / _expr: a running value needs its closing row):
 * 1 <= usable <= T - 1 and T - usable <= KZG_MAX_BLIND_ROWS; rows 0 .. usable hold v[0] .. v[usable]; row `usable` is the
 * closing row and its value is also returned; row usable + 1 + s of column e takes tail_be32[e * (T - usable - 1) + s],
 * canonical scalars, column-major over the recurrences; tail_be32 may be NULL only when usable = T - 1.
 * The n_recs recurrences form, in their order, the rows of ONE new set of the same worker and length; out_commitments48[e]
 * equals kzg_rows_commit(i, n_recs, the T evaluations, T, 1, ..)[e] byte for byte, and *out_handle opens, evaluates, combines,
 * releases, goes stale and counts against KZG_MAX_ROW_SETS (KZG_E_BUSY; KZG_E_NOMEM on a failed allocation, the lane's
 * workspace included) like any other.  A recurrence cannot name another recurrence's output of the same call: compose with a
 * second call.  Each distinct source row named is transformed forward once; nothing row-sized crosses the host link: starts
 * and tails ride in kernel arguments, the closings come back in the copy behind the MSM.
 * WORKSPACE per call: (distinct source rows named + 3) vectors of T elements (A, B and one output vector, reused by every
 * recurrence) and 2 (ceil(n / 4) 3 / 2 + 64) elements for the stacked levels of the scan, 32 bytes per element.
 * Thread safety and "after any error the context keeps serving" are those of kzg_rows_commit_expr.  KZG_E_ARG with a message
 * that begins "recur:" and names the cause: n_recs outside [1, KZG_MAX_BATCH_OPEN]; both expressions of a recurrence empty;
 * n_terms above KZG_MAX_GATE_TERMS; a term of more than KZG_MAX_EXPR_FACTORS factors; a row index at or beyond the
 * concatenation; a coefficient or a start >= r (checked on the HOST, before any lane is taken: an argument error, not a queued
 * failure); a NULL array (start_be32; coeffs_be32 or term_lens of a non-empty expression; term_rows when some term has a
 * factor); T > 2^32; and the usable and tail refusals of the _zk builders.
 * OUT OF SCOPE: second-order recurrences (v[t + 2] from v[t + 1] and v[t]; carry the pair in two columns of a later call, or
 * on the host); a recurrence that runs across calls other than by handing the closing value on as the next `start`; division
 * or an inverse inside a step (compose with KZG_DERIVE_INV0).
 * SOUNDNESS: nothing here is a proof.  The column is prover data: the argument is the caller's gate v(w X) - A v - B in the
 * quotient (kzg_rows_commit_quotient_ext with a rotated factor), restricted to the usable rows where there are blinding rows,
 * plus the boundary gate L_0 (v - start), with every challenge that enters a coefficient drawn after the commitments it depends
 * on are fixed.  A closing value is a convenience for the prover and convinces no verifier.  The library derives no challenge
 * and draws no randomness: the tail must be fresh per proof. */
typedef struct kzg_recurrence {
    kzg_quotient_terms mul;                 /* the multiplier A; n_terms = 0: A = 1 */
    kzg_quotient_terms add;                 /* the addend B; n_terms = 0: B = 0 */
    const uint8_t* start_be32;              /* v[0]: one canonical scalar, 32 bytes */
} kzg_recurrence;
typedef struct kzg_recurrence_opts {
    uint64_t usable;           /* 0: plain layout; else rows 0 .. usable hold v[0] .. v[usable] */
    const uint8_t* tail_be32;  /* n_recs * (T - usable - 1) * 32, column-major; NULL when usable == 0 or usable == T - 1 */
} kzg_recurrence_opts;
int kzg_rows_commit_recurrence(kzg_ctx* ctx, uint32_t n_input_handles, const uint64_t* input_handles,
                               uint32_t n_recs, const kzg_recurrence* recs, const kzg_recurrence_opts* opts /* NULL: plain */,
                               uint8_t* out_commitments48 /* n_recs * 48 */, uint8_t* out_closings32 /* n_recs * 32 */,
                               uint64_t* out_handle);
/* THE FETCHED COLUMNS: a set built FROM sets, every output cell READ OUT OF A TABLE that is already resident -- c = a XOR b from
 * the table (a, b, a ^ b), an S-box output, an opcode's decode flags, any ROM read, no polynomial expression of a and b; the
 * value of a memory read back in program order from the sorted columns (carry the row number through kzg_rows_commit_sorted as
 * a payload column, then fetch by it: the un-sort); v[t] = table[idx[t]].  The concatenated rows of the table_handles sets are
 * the w_tab columns of the table: the first n_keys are the KEY, the n_pay = w_tab - n_keys behind them the PAYLOAD.  The
 * concatenated rows of the input_handles sets are n_reads reads, read-major like the lookups of kzg_rows_commit_multiplicities:
 * read l owns rows l n_keys .. l n_keys + n_keys - 1.  Every cell is a column's value at w_T^t, a canonical field element, as in
 * the sorted and derived calls.
 *   BY KEY (n_keys >= 1): for cell t of read l let q be the SMALLEST table row whose key tuple equals the read's tuple at t in all
 *     n_keys columns.  Output column p of the read takes table[n_keys + p][q].  With flags = KZG_FETCH_INDEX one more column
 *     leads the read's outputs and holds q itself as a field element.  A cell with no such row is a MISS: it gets 0 in every
 *     output column of its read and is counted.
 *   BY ROW INDEX (n_keys = 0): each read owns ONE input row, the address; q is its canonical integer and all w_tab table columns
 *     are payload.  A cell is a miss when q >= the number of addressable table rows; the comparison is on the whole 255-bit
 *     integer (2^32 + 3 or 2^64 is a miss, not row 3 or row 0).  KZG_FETCH_INDEX is refused: the address is the index.
 * The outputs form ONE new set of n_out = n_reads (n_pay + index) rows of the same worker and length, in read order; inside a
 * read the index first, then the payload in table order.  out_commitments48[c] equals kzg_rows_commit(i, n_out, the fetched
 * rows, T, 1, ..)[c] byte for byte, and *out_handle opens, evaluates, combines, releases, goes stale and counts against
 * KZG_MAX_ROW_SETS (KZG_E_BUSY; KZG_E_NOMEM on a failed allocation, the lane's workspace included) like any other.
 * out_missing[l] is the number of misses of read l and out_first_missing[l] the smallest missing row, or KZG_FETCH_NONE -- the
 * mechanism and meaning of out_first of kzg_rows_commit_expr.  A miss is never an error.  The output is a function of the input
 * bytes alone, whatever the device's schedule: a repeated table key answers with its first copy, as the multiplicities call
 * counts on it.
 * opts (NULL: plain layout) is kzg_derive_opts, in layout and refusals: usable = 0 reads all T cells and all T table rows are
 * addressable, tail_be32 must be NULL.  Otherwise 1 <= usable <= T - 1 and T - usable <= KZG_MAX_BLIND_ROWS: cells and table
 * rows at or behind `usable` are never read or matched (as in kzg_rows_commit_multiplicities_zk; by row index an address >=
 * usable is a miss), and output row usable + s of output column c takes tail_be32[c * (T - usable) + s], column-major canonical
 * scalars over the n_out columns.  There is NO closing row.  The tail rides in kernel arguments, the counts come back in the
 * copy behind the MSM; nothing row-sized crosses the host link in either direction.
 * WORKSPACE per call: w_tab + max(n_keys, 1) + n_pay + index vectors of T elements of 32 bytes (the table columns, ONE read's
 * input columns, ONE read's output columns; the reads reuse the last two groups) and, by key, 2 T slots of 4 bytes.
 * Handle lists follow kzg_rows_commit_multiplicities: 1 .. KZG_MAX_BATCH_OPEN handles per list, a handle may repeat and may
 * stand in both lists (the table and the input may be one set), unknown / released / stale -> KZG_E_ARG; every set named must
 * belong to one worker and one (power-of-two) T.  KZG_E_ARG with a message that begins "fetch:" and names the cause: n_reads = 0;
 * n_keys > w_tab; n_pay = 0 without KZG_FETCH_INDEX (nothing to output); an unknown flag; KZG_FETCH_INDEX with n_keys = 0; more
 * than KZG_MAX_BATCH_OPEN table rows, input rows or output rows; an input concatenation that does not hold exactly n_reads
 * max(n_keys, 1) rows; T > 2^27; and the usable and tail refusals of kzg_rows_commit_derived.  The source sets are only read; a
 * release or an SRS load racing the call follows the rules of kzg_rows_open.  Thread-safe like every call; after any error the
 * context keeps serving.
 * OUT OF SCOPE: per-read selectors (a disabled cell is a counted miss that reads 0: multiply by the selector with
 * kzg_rows_commit_expr afterwards); a default value other than 0; the LAST matching row instead of the first; tables longer or
 * shorter than the input rows.  (A bitwise or arithmetic operation on machine words needs no 2^(2b)-row table to be COMPUTED:
 * kzg_rows_commit_int below builds the witness column directly; the table stays the caller's argument for it.)
 * SOUNDNESS: nothing here is a proof.  The fetched rows are prover data; the argument is the lookup of the tuple (key, payload)
 * in the table (kzg_rows_commit_multiplicities -> kzg_rows_commit_lookup_sum -> the quotient's logUp relation), with theta and
 * beta drawn AFTER these commitments are fixed.  A zero miss count is a convenience for the prover and convinces no verifier.
 * The library derives no challenge and draws no randomness: the tail must be fresh per proof. */
#define KZG_FETCH_INDEX 1u                  /* flags: lead every read's outputs with the matching row number */
#define KZG_FETCH_NONE  0xffffffffffffffffull
int kzg_rows_commit_fetch(kzg_ctx* ctx, uint32_t n_input_handles, const uint64_t* input_handles,
                          uint32_t n_table_handles, const uint64_t* table_handles, uint32_t n_reads, uint32_t n_keys,
                          uint32_t flags /* 0 or KZG_FETCH_INDEX */, const kzg_derive_opts* opts /* NULL: plain */,
                          uint8_t* out_commitments48 /* n_out * 48 */, uint64_t* out_missing /* n_reads */,
                          uint64_t* out_first_missing /* n_reads */, uint64_t* out_handle);
/* THE SIGMA COLUMNS: a set built FROM sets, the permutation rows that kzg_rows_commit_grand_product* takes as "already
 * resident", built on the device from VARIABLE LABELS -- the shape in which every frontend holds its copy constraints: one id
 * per wire slot, where a copy constraint is "same id" (commit the ids with kzg_rows_commit_typed).  The concatenated rows of the
 * label_handles sets are k label columns l_0 .. l_{k-1}, 1 <= k <= KZG_MAX_BATCH_OPEN.  With w_T = 7^((r-1)/T), natural order --
 * exactly the convention of kzg_rows_commit_grand_product -- cell (c, t) carries the label l_c(w_T^t), taken as its CANONICAL
 * INTEGER in [0, r); any field element is a label.  Cells with equal labels are one copy class.
 * Let n = opts->usable, or n = T for the plain layout.  The cells with t < n take part; their flat index is j = c T + t.  The
 * call builds the permutation sigma in which each class is ONE CYCLE IN ASCENDING FLAT INDEX: a cell maps to the next larger
 * flat index of its class, the largest to the smallest; and writes sigma_c(w_T^t) = shifts[c'] w_T^t' for the image (c', t').
 * Two kinds of cell map to themselves:
 *   FREE CELLS: a participating cell whose label equals opts->free_label_be32 (NULL: no such label) maps to itself, whatever
 *     else carries that label.  With KZG_COL_I32 label columns the natural choice is -1, which is r - 1.
 *   ROWS t >= n: sigma_c(w_T^t) = shifts[c] w_T^t.  Their labels are never read.  sigma is a public fixed column: there is no
 *     tail and no closing row, and therefore no bound T - usable <= KZG_MAX_BLIND_ROWS as the _zk builders have.
 * The result is a new set of k rows of the same worker and length: out_commitments48[c] equals kzg_rows_commit(i, k, the sigma
 * evaluations, T, 1, ..)[c] byte for byte, and *out_handle opens, evaluates, combines, releases, goes stale and counts against
 * KZG_MAX_ROW_SETS (KZG_E_BUSY; KZG_E_NOMEM on a failed allocation, the lane's workspace included: 2 k + 1 T-element vectors
 * and about a third of k more for the sort) like any other.  out_stats[0] is the number of classes (distinct non-free labels
 * among the participating cells), out_stats[1] the number of participating cells that map to themselves (free cells and
 * singletons).  The output is a function of the input bytes alone, whatever the device's schedule.  The shifts ride in kernel
 * arguments and the stats come back in the copy behind the MSM; nothing row-sized crosses the host link in either direction.
 * Handle lists follow kzg_rows_commit_sorted: 1 .. KZG_MAX_BATCH_OPEN handles, a handle may repeat (two equal label columns),
 * unknown / released / stale -> KZG_E_ARG.  KZG_E_ARG with a message that names the cause: k = 0 or k > KZG_MAX_BATCH_OPEN; a
 * concatenation that does not hold exactly k rows; sets of several workers or several T; usable >= T; a shift or the free
 * label >= r; k n > 2^27 (the sort's bound: positions are 32-bit).  The source sets are only read; a release or an SRS load
 * racing the call follows the rules of kzg_rows_open.  Thread-safe like every call; after any error the context keeps serving.
 * OUT OF SCOPE: building the wire columns from a variable vector (a = w[id] with more variables than rows: see
 * kzg_rows_commit_fetch by row index for up to T variables); labels that arrive as typed host buffers without a set; copy
 * constraints given as equality pairs (union-find); one permutation chained across more than KZG_MAX_BATCH_OPEN columns in one
 * call (label per chunk and use kzg_rows_commit_grand_product_chain).
 * SOUNDNESS: nothing here is a proof.  sigma is a fixed column of the circuit, part of the verifying key; the copy argument is
 * the grand product over it (kzg_rows_commit_grand_product*, beta and gamma drawn AFTER the wire commitments are fixed).  The
 * shifts must put the k cosets shifts[c] H apart (1, 7, 49, .. do), which the library does not check. */
typedef struct kzg_sigma_opts {
    uint64_t usable;                 /* 0: all T rows take part; else rows [0, usable), 1 <= usable <= T - 1 */
    const uint8_t* free_label_be32;  /* NULL: none */
} kzg_sigma_opts;
int kzg_rows_commit_sigma(kzg_ctx* ctx, uint32_t n_label_handles, const uint64_t* label_handles, uint32_t k,
                          const uint8_t* shifts_be32 /* k*32 */, const kzg_sigma_opts* opts /* NULL: plain, no free label */,
                          uint8_t* out_commitments48 /* k*48 */, uint64_t out_stats[2], uint64_t* out_handle);
/* THE COPY CHECK: "does this witness respect its copy constraints?", answered cell by cell on the device.  The label arguments
 * and opts are those of kzg_rows_commit_sigma; the concatenated rows of the wire_handles sets are the k wire columns, cell for
 * cell beside the labels.  A participating, non-free cell is a VIOLATION when its value differs from the value of its class's
 * smallest-flat-index cell.  out[0] is the number of violations, out[1] the smallest violating flat index c T + t, or
 * UINT64_MAX if there is none.  No set is created and no inverse transform or MSM runs (as a kzg_rows_commit_expr call made of
 * checks alone).  The two handle lists follow kzg_rows_commit_fetch (a handle may stand in both); the refusals are those of
 * kzg_rows_commit_sigma, with both concatenations holding exactly k rows of one worker and one T.
 * SOUNDNESS: a violation count is a convenience for the prover and convinces no verifier.  The argument is the grand product
 * over the sigma of kzg_rows_commit_sigma. */
int kzg_rows_check_copies(kzg_ctx* ctx, uint32_t n_wire_handles, const uint64_t* wire_handles, uint32_t n_label_handles,
                          const uint64_t* label_handles, uint32_t k, const kzg_sigma_opts* opts /* NULL: plain, no free label */,
                          uint64_t out[2]);
/* THE INTEGER ALU COLUMNS: a set built FROM sets, the witness columns of machine-word arithmetic -- what a zkVM-style execution
 * trace holds beside its field arithmetic (kzg_rows_commit_expr): bitwise results, carries, borrows, high products, quotients
 * and remainders, shifted halves.  The concatenated rows of the input_handles sets (as in kzg_rows_open) are the source
 * columns; cell t of a column is its value at w_T^t, taken as its CANONICAL INTEGER in [0, r), exactly as in
 * kzg_rows_commit_derived.  Each of the n_ops ops has a kind, a width w in [1, 64] with M = 2^w, a first operand row a, a second
 * operand that is the row b or, with KZG_INT_IMM in flags, the 64-bit immediate imm, and `count`, its number of output rows.
 * READING AN OPERAND: an operand cell x >= 2^w is OUT OF RANGE: the op uses x mod 2^w, its low w bits.  Such a cell is counted
 * once in out_counts[op], however many of its operands are out of range, and out_first[op] is the smallest such row, or
 * KZG_INT_NONE.  An out-of-range cell is never an error; the output rows are still written.  An immediate >= 2^w (SPLIT: an
 * immediate > w) is KZG_E_ARG.  The output rows of an op, in this order (count selects the first one or both):
 *   KZG_INT_AND, _OR, _XOR (count 1)   a op b
 *   KZG_INT_ADD    (count 1 or 2)      (a + b) mod M;  the carry (a + b) >> w, 0 or 1
 *   KZG_INT_SUB    (count 1 or 2)      (a - b) mod M;  the borrow, 1 where a < b and else 0 (the unsigned less-than bit)
 *   KZG_INT_MUL    (count 1 or 2)      (a b) mod M;    (a b) >> w
 *   KZG_INT_DIVMOD (count 1 or 2)      floor(a / b), M - 1 where b = 0;  a mod b, a where b = 0 (the RISC-V convention; a zero
 *                                      divisor is neither counted nor an error)
 *   KZG_INT_SPLIT  (count 1 or 2)      a >> s;  a mod 2^s.  The second operand is the shift s: an immediate in [0, w], or a row
 *                                      whose cell is s; a cell with s > w is out of range and is taken as s = w.  Every shift and
 *                                      rotation follows by composition: shl = lo 2^s, rotr = lo 2^(w - s) + hi through
 *                                      kzg_rows_commit_expr.
 * A row may serve as both operands of one op.  n_ops <= KZG_MAX_BATCH_OPEN and n_out = sum of the counts, 1 <= n_out <=
 * KZG_MAX_BATCH_OPEN.  All outputs of a call form ONE new set of the same worker and length, in the order of ops:
 * out_commitments48[c] equals kzg_rows_commit(i, n_out, these rows, T, 1, ..)[c] byte for byte, and *out_handle opens,
 * evaluates, combines, releases, goes stale and counts against KZG_MAX_ROW_SETS (KZG_E_BUSY; KZG_E_NOMEM on a failed allocation,
 * the lane's workspace included: one T-element vector per DISTINCT source row, which is transformed once however many ops name
 * it, and one per output row) like any other.  ONE kernel launch computes every op of the call; the counts and first rows come
 * back in the copy behind the MSM; nothing row-sized crosses the host link in either direction.
 * opts (NULL: plain layout) is kzg_derive_opts, exactly as kzg_rows_commit_derived reads it: source rows t >= usable are never
 * read or counted, output row usable + s of output column c takes tail_be32[c * (T - usable) + s], there is NO closing row.
 * Handle lists follow kzg_rows_open.  KZG_E_ARG with a message that begins "int:" and names the cause: n_ops = 0 or n_ops >
 * KZG_MAX_BATCH_OPEN; n_out > KZG_MAX_BATCH_OPEN; an unknown kind; an unknown flag; w outside [1, 64]; count outside the kind's
 * set; a row at or beyond the concatenation; an immediate that does not fit; the usable and tail refusals of
 * kzg_rows_commit_derived; the handle refusals of kzg_rows_open.  The source sets are only read; a release or an SRS load racing
 * the call follows the rules of kzg_rows_open.  Thread-safe like every call; after any error the context keeps serving.
 * OUT OF SCOPE: signed variants (sra, mulh, signed div / rem, slt: the caller adds the bias 2^(w-1) and corrects with
 * kzg_rows_commit_expr); widths above 64; three-operand ops (a b + c, funnel shifts); per-row selectors (an op-code column
 * choosing the kind per row: build every candidate and select with kzg_rows_commit_expr); a separate count of zero divisors.
 * (Both in ONE call, the signed kinds and a kind chosen per row by an op-code column: kzg_rows_commit_alu below.)
 * (Widths above 64 as limbs, and a b + c mod m: kzg_rows_commit_wide below.)
 * SOUNDNESS: nothing here is a proof.  The rows are prover data; the argument is the caller's gates plus the range lookups of
 * the outputs (kzg_rows_commit_derived LIMBS -> kzg_rows_commit_multiplicities -> kzg_rows_commit_lookup_sum): a + b = s + carry M;
 * a - b = d - borrow M; a b = lo + hi M; a = q b + rem with rem < b shown through the borrow of a SUB (and the b = 0 case
 * through an is-zero bit); a = hi 2^s + lo with lo < 2^s, where for a per-row s the power 2^s is fetched from a table
 * (kzg_rows_commit_fetch); a bitwise op through its 2^(2b)-row table on the limbs.  Every challenge is drawn AFTER these
 * commitments are fixed.  A zero out-of-range count is a convenience for the prover and convinces no verifier.  The library
 * derives no challenge and draws no randomness: the tail must be fresh per proof. */
#define KZG_INT_AND    1
#define KZG_INT_OR     2
#define KZG_INT_XOR    3
#define KZG_INT_ADD    4
#define KZG_INT_SUB    5
#define KZG_INT_MUL    6
#define KZG_INT_DIVMOD 7
#define KZG_INT_SPLIT  8
#define KZG_INT_IMM    1u                   /* flags: the second operand is `imm`, not row b */
#define KZG_INT_NONE   0xffffffffffffffffull
typedef struct kzg_int_op {
    uint32_t kind;   /* KZG_INT_* */
    uint32_t width;  /* w in [1, 64] */
    uint32_t a;      /* first operand: a row, index into the concatenated rows of input_handles */
    uint32_t b;      /* second operand: a row (a SPLIT's shift column); must be 0 with KZG_INT_IMM */
    uint64_t imm;    /* second operand with KZG_INT_IMM: below 2^w (SPLIT: at most w); must be 0 without */
    uint32_t flags;  /* 0 or KZG_INT_IMM */
    uint32_t count;  /* output rows: 1, or 2 where the kind has a second row */
} kzg_int_op;
int kzg_rows_commit_int(kzg_ctx* ctx, uint32_t n_input_handles, const uint64_t* input_handles, uint32_t n_ops,
                        const kzg_int_op* ops, const kzg_derive_opts* opts /* NULL: plain */,
                        uint8_t* out_commitments48 /* n_out * 48 */, uint64_t* out_counts /* n_ops */,
                        uint64_t* out_first /* n_ops */, uint64_t* out_handle);
/* THE ALU COLUMN WITH AN OP-CODE COLUMN: kzg_rows_commit_int with the kind chosen PER ROW, the shape of a CPU table in a zkVM
 * trace -- one result column, and an op-code column that says per row whether the row is an add, an sltu, an sra or a mulh.
 * `program` has n_entries <= KZG_ALU_MAX_PROGRAM entries and the entry's index is the op-code.  An entry is idle (kind
 * KZG_ALU_IDLE, every other field 0) or gives a kind, a width w in [1, 64] with M = 2^w, and, with KZG_ALU_IMM in flags, an
 * immediate second operand imm.  Each of the n_units <= KZG_ALU_MAX_UNITS units names three rows of the concatenated rows of
 * the input_handles sets (as in kzg_rows_open) -- the op-code column op_row and the operand columns a and b; one row may serve
 * several roles, one program serves all units -- and `count`, 1 or 2, its number of output rows.  Cells are CANONICAL INTEGERS
 * as in kzg_rows_commit_int.  Per cell t, with c the integer of op_row[t]:
 *   c >= n_entries (a cell at or above 2^32 included)   UNKNOWN: the outputs are 0; counted in out_unknown[unit], the smallest
 *                                                       such row in out_first_unknown[unit] (KZG_ALU_NONE: none)
 *   program[c] idle                                     the outputs are 0; nothing else is read, nothing is counted (the row of a
 *                                                       load or a branch in a CPU table)
 *   otherwise                                           a and b are reduced to their low w bits exactly as in kzg_rows_commit_int:
 *                                                       a cell with an operand at or above 2^w is counted ONCE in
 *                                                       out_counts[unit], the smallest such row is out_first[unit] (KZG_ALU_NONE:
 *                                                       none); it is never an error.  With KZG_ALU_IMM the second operand is imm
 *                                                       and column b is neither read nor counted for that row
 * The output rows (count selects row 0 alone or both), with sgn(x) = x - M [x >= M / 2] and, for the five shifts and
 * rotations, s = b mod w (the RISC-V rule at w = 32 and 64: a shift amount is never out of range on its own):
 *   KZG_ALU_AND .. KZG_ALU_SPLIT   the numbers and the exact rows of KZG_INT_AND .. KZG_INT_SPLIT, SPLIT's clamp-and-count of a
 *                                  shift above w included; row 1 of AND, OR and XOR, which have none there, is 0
 *   KZG_ALU_LTU      [a < b];                                   (a - b) mod M
 *   KZG_ALU_LT       [sgn a < sgn b];                           (a - b) mod M
 *   KZG_ALU_EQ       [a = b];                                   (a - b) mod M
 *   KZG_ALU_SLL      (a 2^s) mod M;                             a >> (w - s), 0 where s = 0
 *   KZG_ALU_SRL      a >> s;                                    a mod 2^s
 *   KZG_ALU_SRA      floor(sgn a / 2^s) mod M;                  a mod 2^s
 *   KZG_ALU_ROTL     SLL's row 0 + SLL's row 1;                 a >> (w - s), 0 where s = 0
 *   KZG_ALU_ROTR     (a >> s) + (a mod 2^s) 2^(w - s), a where s = 0;   a mod 2^s
 *   KZG_ALU_MULHU    (a b) >> w;                                (a b) mod M
 *   KZG_ALU_MULH     floor(sgn a sgn b / M) mod M;              (a b) mod M
 *   KZG_ALU_MULHSU   floor(sgn a b / M) mod M;                  (a b) mod M
 *   KZG_ALU_DIV      q = trunc(sgn a / sgn b) mod M;            (sgn a - q sgn b) mod M.  The RISC-V convention: b = 0 gives M - 1
 *                                                               and a; a = M / 2 with b = M - 1 (the overflow) gives M / 2 and 0;
 *                                                               neither is counted, neither is an error
 *   KZG_ALU_REM      DIV's row 1;                               DIV's row 0
 *   KZG_ALU_REMU     a mod b, a where b = 0;                    floor(a / b), M - 1 where b = 0
 *   KZG_ALU_SEXT     the low f bits of a sign-extended to w bits;   bit f - 1 of a.  f is the second operand: a column cell of 0
 *                                                               or above w is out of range, taken as w and counted
 * All of it is defined at w = 1 (sgn 1 = -1, s = 0).  An immediate must be below 2^w; SPLIT's and SEXT's at most w, SEXT's not 0.
 * count = 2 needs an entry whose kind has a second row (a program of AND, OR and XOR entries alone refuses it).  n_out = the sum
 * of the counts <= KZG_MAX_BATCH_OPEN.  All outputs form ONE new set of the same worker and length, unit by unit, row 0 then
 * row 1: out_commitments48[c] equals kzg_rows_commit(i, n_out, these rows, T, 1, ..)[c] byte for byte.  ONE kernel launch
 * computes every unit; each DISTINCT source row is transformed once; the four statistics of every unit come back in the copy
 * behind the MSM; nothing row-sized crosses the host link.  opts (usable / tail), the handle rules, staleness,
 * KZG_MAX_ROW_SETS, KZG_E_BUSY / KZG_E_NOMEM and thread safety are exactly those of kzg_rows_commit_int.  KZG_E_ARG with a
 * message that begins "alu:" and names the cause: n_entries outside [1, KZG_ALU_MAX_PROGRAM]; n_units outside [1,
 * KZG_ALU_MAX_UNITS]; an unknown kind; an unknown flag; an idle entry with a field set; w outside [1, 64]; an immediate that
 * does not fit, or one given without KZG_ALU_IMM; count outside {1, 2}, or 2
 * without a two-row kind; n_out > KZG_MAX_BATCH_OPEN; a row at or beyond the concatenation; the usable, tail and handle refusals
 * of kzg_rows_commit_int.  After any error the context keeps serving.
 * OUT OF SCOPE: widths above 64; three-operand ops; a per-row width column (the width comes from the program entry); a per-row
 * count; Zbb-style bit counts (clz, ctz, popcount) and min / max; more than KZG_ALU_MAX_PROGRAM op-codes or KZG_ALU_MAX_UNITS
 * units per call; a separate count of zero divisors or overflows; any proof.
 * SOUNDNESS: nothing here is a proof.  The rows are prover data; the argument is the caller's gates, each multiplied by the
 * selector of its op-code, plus the range lookups of the outputs (as for kzg_rows_commit_int): LTU, LT, EQ: a - b = d - borrow M
 * with the sign bits of a and b split off for LT, and d inv0(d) for EQ; SLL, ROTL: a 2^s = hi M + lo; SRL, SPLIT, ROTR: a = hi
 * 2^s + lo with lo < 2^s; SRA: sgn(hi) 2^s + lo = sgn a; MULHU: a b = hi M + lo; MULH: sgn a sgn b = sgn(hi) M + lo; MULHSU:
 * sgn a b = sgn(hi) M + lo; DIV, REM: sgn a = sgn q sgn b + sgn r with |r| < |b| and r = 0 or of a's sign, the zero divisor and
 * the overflow through their is-zero bits; REMU: a = q b + r with r < b; SEXT: x = lo + bit (M - 2^f) with lo < 2^f and bit its
 * top bit; 2^s for a per-row s fetched from a table (kzg_rows_commit_fetch).  Every challenge is drawn AFTER these commitments
 * are fixed.  Zero counts are a convenience for the prover and convince no verifier.  The library derives no challenge and
 * draws no randomness: the tail must be fresh per proof. */
#define KZG_ALU_IDLE   0
#define KZG_ALU_AND    1
#define KZG_ALU_OR     2
#define KZG_ALU_XOR    3
#define KZG_ALU_ADD    4
#define KZG_ALU_SUB    5
#define KZG_ALU_MUL    6
#define KZG_ALU_DIVMOD 7
#define KZG_ALU_SPLIT  8
#define KZG_ALU_LTU    9
#define KZG_ALU_LT     10
#define KZG_ALU_EQ     11
#define KZG_ALU_SLL    12
#define KZG_ALU_SRL    13
#define KZG_ALU_SRA    14
#define KZG_ALU_ROTL   15
#define KZG_ALU_ROTR   16
#define KZG_ALU_MULHU  17
#define KZG_ALU_MULH   18
#define KZG_ALU_MULHSU 19
#define KZG_ALU_DIV    20
#define KZG_ALU_REM    21
#define KZG_ALU_REMU   22
#define KZG_ALU_SEXT   23
#define KZG_ALU_IMM    1u                   /* flags: the entry's second operand is `imm`, not column b */
#define KZG_ALU_NONE   0xffffffffffffffffull
#define KZG_ALU_MAX_PROGRAM 64
#define KZG_ALU_MAX_UNITS   8
typedef struct kzg_alu_entry {
    uint32_t kind;   /* KZG_ALU_IDLE or a kind KZG_ALU_AND .. KZG_ALU_SEXT */
    uint32_t width;  /* w in [1, 64]; 0 on an idle entry */
    uint64_t imm;    /* second operand with KZG_ALU_IMM: below 2^w (SPLIT, SEXT: at most w; SEXT: not 0); must be 0 without */
    uint32_t flags;  /* 0 or KZG_ALU_IMM */
    uint32_t pad;    /* must be 0 */
} kzg_alu_entry;
typedef struct kzg_alu_unit {
    uint32_t op_row; /* the op-code column: a row, index into the concatenated rows of input_handles */
    uint32_t a;      /* first operand column */
    uint32_t b;      /* second operand column (read only on rows whose entry has no immediate) */
    uint32_t count;  /* output rows: 1 or 2 */
} kzg_alu_unit;
int kzg_rows_commit_alu(kzg_ctx* ctx, uint32_t n_input_handles, const uint64_t* input_handles, uint32_t n_entries,
                        const kzg_alu_entry* program, uint32_t n_units, const kzg_alu_unit* units,
                        const kzg_derive_opts* opts /* NULL: plain */, uint8_t* out_commitments48 /* n_out * 48 */,
                        uint64_t* out_counts /* n_units */, uint64_t* out_first /* n_units */, uint64_t* out_unknown /* n_units */,
                        uint64_t* out_first_unknown /* n_units */, uint64_t* out_handle);
/* THE MULTI-LIMB INTEGER COLUMNS: a set built FROM sets, the witness columns of 256-bit, 384-bit and 512-bit arithmetic -- uint256
 * mul / div, a b + c mod p over the base fields of secp256k1, bn254 and BLS12-381 -- which kzg_rows_commit_int and
 * kzg_rows_commit_alu leave out (widths above 64, three operands).  The concatenated rows of the input_handles sets (as in
 * kzg_rows_open) are the source columns.  A WIDE VALUE is L consecutive rows of them: limb l is row first + l, little-endian,
 * the order in which kzg_rows_commit_derived's LIMBS writes its rows.  Cell t of a limb row is taken as its CANONICAL INTEGER in
 * [0, r) and reduced to its low b bits; the value at row t is sum_l limb_l[t] 2^(b l).  1 <= b <= 64, 1 <= L <= 8, W = b L <=
 * 512.  A limb cell at or above 2^b is OUT OF RANGE: it is reduced, never refused; a row t with such a limb in any operand is
 * counted ONCE in out_counts[op], and out_first[op] is the smallest such row, or KZG_INT_NONE.  An immediate (imm_be64, m_be64)
 * is a big-endian integer of 64 bytes and must be below 2^W.  An operand field holds the first row of the value, or
 * KZG_WIDE_ABSENT.  The output rows of an op, in this order (count selects the first part or all):
 *   KZG_WIDE_ADD    (count L or L + 1)  (a + b) mod 2^W as L limbs; the carry, 0 or 1
 *   KZG_WIDE_SUB    (count L or L + 1)  (a - b) mod 2^W as L limbs; the borrow, 1 where a < b
 *   KZG_WIDE_MUL    (count L or 2 L)    the low L limbs of a b; the high L limbs
 *   KZG_WIDE_DIVMOD (count L or 2 L)    floor(a / b) as L limbs; a mod b as L limbs.  Where b = 0: 2^W - 1 and a, the convention
 *                                       of kzg_rows_commit_int, neither counted nor an error
 *   KZG_WIDE_MULMOD (count L or 2 L)    with t = a b + d and the modulus m = m_be64, 1 <= m < 2^W: r = t mod m as L limbs; q =
 *                                       floor(t / m) as L limbs.  b is a wide row, the immediate imm_be64 (KZG_WIDE_IMM_B), or
 *                                       absent (then 1).  d = 0 without an operand c, d = c with one.  With KZG_WIDE_NEG_C: d = m -
 *                                       (c mod m), which is m where c = 0 or there is no c, and a row with c > m is counted out of
 *                                       range: the caller's gate is a b + m - c = q m + r, and q is never negative.  A row with q
 *                                       >= 2^W (operands not reduced against a small m) writes the low W bits of q and is counted
 *                                       in out_qover[op], the smallest such row in out_first_qover[op] (or KZG_INT_NONE)
 *   KZG_WIDE_CARRY  (count 2 L - 1)     the carry columns of the limb identity of a MULMOD whose q and r are resident: operands
 *                                       a, b, c as for MULMOD, q, r (wide rows) and m; the limbs of m and d come from the integers
 *                                       m and d cut into b-bit limbs.  For k = 0 .. 2 L - 1:
 *                                         s_k = sum_{i + j = k} (A_i B_j - Q_i M_j) + [k < L] (D_k - R_k) + carry_(k-1),
 *                                         carry_(-1) = 0, carry_k = floor(s_k / 2^b), rounding towards minus infinity.
 *                                       The rows are carry_0 .. carry_(2L-2); a negative carry x is the cell r - |x|, the
 *                                       convention of the typed i64 columns.  b <= 56, so every carry fits a signed 64-bit word.
 *                                       A row where some s_k is no multiple of 2^b, or carry_(2L-1) != 0, is INEXACT: counted in
 *                                       out_qover[op] / out_first_qover[op]; its rows are still written
 * The other kinds take b as a row or an immediate and no c, q, r or m (all zero bytes).  A row may serve several operands of one
 * op.  1 <= n_ops <= KZG_WIDE_MAX_OPS and n_out = the sum of the counts, 1 <= n_out <= KZG_MAX_BATCH_OPEN.  All outputs of a call
 * form ONE new set of the same worker and length, in the order of ops: out_commitments48[c] equals kzg_rows_commit(i, n_out,
 * these rows, T, 1, ..)[c] byte for byte, and *out_handle opens, evaluates, combines, releases, goes stale and counts against
 * KZG_MAX_ROW_SETS (KZG_E_BUSY; KZG_E_NOMEM on a failed allocation, the lane's workspace included: one T-element vector per
 * DISTINCT source row named and one per output row) like any other.  ONE kernel launch computes every op of the call; the four
 * statistics come back in the copy behind the MSM; nothing row-sized crosses the host link in either direction.
 * opts (NULL: plain layout) is kzg_derive_opts, exactly as kzg_rows_commit_derived reads it: source rows t >= usable are never
 * read or counted, output row usable + s of output column c takes tail_be32[c * (T - usable) + s], there is NO closing row.
 * Handle lists follow kzg_rows_open.  KZG_E_ARG with a message that begins "wide:" and names the cause: n_ops outside [1,
 * KZG_WIDE_MAX_OPS]; n_out outside [1, KZG_MAX_BATCH_OPEN]; an unknown kind; an unknown flag; b outside [1, 64] (CARRY: [1, 56]),
 * L outside [1, 8], W above 512; a count outside the kind's set; an operand whose L rows reach beyond the concatenation; an
 * operand, immediate, modulus or flag that the kind does not take, or a missing one that it needs; an immediate or a modulus at
 * or above 2^W; m = 0; the usable and tail refusals of kzg_rows_commit_derived; the handle refusals of kzg_rows_open.  The
 * source sets are only read; a release or an SRS load racing the call follows the rules of kzg_rows_open.  Thread-safe like
 * every call; after any error the context keeps serving.
 * OUT OF SCOPE: L > 8 (regroup 8-bit or 16-bit limbs into wider ones with kzg_rows_commit_expr, or cut the outputs again with
 * kzg_rows_commit_derived); a per-row modulus; modular inversion and division (no longer missing: they have their own call, the DIV unit of
 * kzg_rows_commit_ec, for an odd modulus of up to 256 bits); signed operands; an op-code column; operands
 * on DISTINCT rows beyond the KZG_MAX_BATCH_OPEN concatenated rows a call reads: the limit counts rows, not L, and a row may
 * serve several operands, so a CARRY runs at any L <= 8, but with a, q and r on three distinct runs of rows it has L <= 5 (L <=
 * 4 with b as a fourth).  A 256-bit or 384-bit carry chain over distinct a, q, r is therefore not to be had in one call.
 * SOUNDNESS: nothing here is a proof.  The rows are prover data; the argument is the caller's gates over the limbs plus the
 * range lookups of every output limb and carry: the limb identity s_k = carry_k 2^b for k < 2 L (kzg_rows_commit_expr over the
 * operand, quotient, remainder and carry columns), r < m through a SUB and its borrow, and for a modular statement W large
 * enough that the integer identity cannot wrap in the field.  Every challenge is drawn AFTER these commitments are fixed.  Zero
 * counts are a convenience for the prover and convince no verifier.  The library derives no challenge and draws no randomness:
 * the tail must be fresh per proof. */
#define KZG_WIDE_ADD    1
#define KZG_WIDE_SUB    2
#define KZG_WIDE_MUL    3
#define KZG_WIDE_DIVMOD 4
#define KZG_WIDE_MULMOD 5
#define KZG_WIDE_CARRY  6
#define KZG_WIDE_IMM_B  1u                  /* flags: operand b is imm_be64 */
#define KZG_WIDE_NEG_C  2u                  /* flags (MULMOD, CARRY): d = m - (c mod m) */
#define KZG_WIDE_ABSENT 0xffffffffu         /* an operand field without a row */
#define KZG_WIDE_MAX_OPS 8
#define KZG_WIDE_MAX_LIMBS 8
typedef struct kzg_wide_op {
    uint32_t kind;          /* KZG_WIDE_* */
    uint32_t bits;          /* b in [1, 64]; CARRY: [1, 56] */
    uint32_t limbs;         /* L in [1, 8], b L <= 512 */
    uint32_t count;         /* output rows: see the kinds */
    uint32_t flags;         /* 0, KZG_WIDE_IMM_B, KZG_WIDE_NEG_C or both */
    uint32_t a, b, c, q, r; /* the first row of each operand in the concatenated rows of input_handles, or KZG_WIDE_ABSENT */
    uint8_t imm_be64[64];   /* operand b with KZG_WIDE_IMM_B: below 2^W; all zero without */
    uint8_t m_be64[64];     /* the modulus of MULMOD and CARRY: in [1, 2^W); all zero on the other kinds */
} kzg_wide_op;
int kzg_rows_commit_wide(kzg_ctx* ctx, uint32_t n_input_handles, const uint64_t* input_handles, uint32_t n_ops,
                         const kzg_wide_op* ops, const kzg_derive_opts* opts /* NULL: plain */,
                         uint8_t* out_commitments48 /* n_out * 48 */, uint64_t* out_counts /* n_ops */,
                         uint64_t* out_first /* n_ops */, uint64_t* out_qover /* n_ops */, uint64_t* out_first_qover /* n_ops */,
                         uint64_t* out_handle);
/* THE POSEIDON PERMUTATION COLUMNS: a set built FROM sets, the columns of the hash chip -- Merkle nodes, page commitments,
 * in-circuit Fiat-Shamir -- which kzg_rows_commit_expr (no row-to-row dependence) and kzg_rows_commit_recurrence (affine in the
 * running value) cannot express.  The library generates NO constants: the caller supplies the state width t, 2 <= t <= 8, the
 * number of full rounds R_F (even, 2 <= R_F <= 16) and of partial rounds R_P (0 <= R_P <= 128), the t R round constants rc
 * (round-major, R = R_F + R_P) and the t x t matrix M (row-major), all canonical scalars of 32 big-endian bytes.  The S-box is
 * x -> x^5.  THE PERMUTATION of a state s, for each round rho = 0 .. R - 1:
 *   1. s_i += rc[rho t + i] for every i;
 *   2. s_i <- s_i^5 for every i where rho < R_F / 2 or rho >= R_F / 2 + R_P (a full round), else for i = 0 only;
 *   3. s <- M s, that is s'_i = sum_j M[i t + j] s_j.
 * This is the plain (unoptimised) Hades schedule.  The concatenated rows of the input_handles sets (as in kzg_rows_open) are the
 * source columns.  A call has 1 <= n_units <= KZG_POSEIDON_MAX_UNITS units that share params.  in[j], j < t, is the source row of
 * state element j, or KZG_POSEIDON_IMM: then the element is imm_be32[j] on every row (a domain tag, the capacity element,
 * padding), canonical; imm_be32[j] is all zero beside a row.  One row may serve several slots.  With n = opts->usable, or T in
 * the plain layout:
 *   KZG_POSEIDON_ROW     for every row t' < n the state is (in_0[t'], .., in_{t-1}[t']); output column c, c < n_out, holds state
 *                        element out[c] after the permutation; 1 <= n_out <= t, the out[c] distinct and below t.  With the flag
 *                        KZG_POSEIDON_CHECK the unit commits NOTHING: expect[c] is the source row that column c is compared
 *                        with, out_mismatch[u] is the number of rows t' < n where some expected cell differs from the computed
 *                        one and out_first_mismatch[u] the smallest such row, or KZG_POSEIDON_NONE
 *   KZG_POSEIDON_ROUNDS  the round trace with the period P = period >= R + 1: block b = 0 .. floor(n / P) - 1 occupies rows
 *                        [b P, b P + P); its input is read at row b P of the in entries; output column j (n_out = t, out[j] = j)
 *                        holds at row b P + rho state element j BEFORE round rho, rho = 0 .. R, so row b P is the input and row
 *                        b P + R the permutation's output; rows b P + R + 1 .. b P + P - 1 and the rows from floor(n / P) P to
 *                        n - 1 are 0.  No source cell is read other than at the rows b P of existing blocks; a block cut by n is
 *                        not started.  KZG_POSEIDON_CHECK is refused
 * out_perms[u] is the number of permutations unit u ran: n for a ROW unit, floor(n / P) for a ROUNDS unit; out_mismatch[u] = 0
 * and out_first_mismatch[u] = KZG_POSEIDON_NONE on a unit that commits.  All committed columns of a call form ONE new set of the
 * same worker and length, in the order of units, then of out: out_commitments48[c] equals kzg_rows_commit(i, n_out, these rows,
 * T, 1, ..)[c] byte for byte, and *out_handle opens, evaluates, combines, releases, goes stale and counts against
 * KZG_MAX_ROW_SETS like any other.  A call made of checks alone creates no set (*out_handle = 0, out_commitments48 may be null),
 * runs no inverse transform and no MSM and counts nothing against KZG_MAX_ROW_SETS: the convention of kzg_rows_commit_expr's
 * checks and of kzg_rows_check_copies.  ONE kernel launch computes every unit; the constants reach the device through a buffer
 * of the lane; nothing row-sized crosses the host link.  A call reads at most KZG_MAX_BATCH_OPEN distinct rows and commits at
 * most KZG_MAX_BATCH_OPEN.  opts (NULL: plain layout) is kzg_derive_opts as kzg_rows_commit_derived reads it: source rows t' >=
 * usable are never read, compared or counted, output row usable + s of committed column c takes tail_be32[c * (T - usable) + s],
 * there is NO closing row.  Handle lists, worker, T, staleness and threads follow kzg_rows_commit_expr.  KZG_E_ARG with a message
 * that begins "poseidon:" and names the cause: t, R_F (an odd one included), R_P, a period below R + 1 or n_units outside their
 * ranges; more than KZG_MAX_BATCH_OPEN output rows or distinct input rows; a constant, matrix entry or immediate at or above r
 * (checked on the host before a lane is taken); an unknown mode or flag; n_out outside [1, t], an out index at or above t or a
 * repeated one; KZG_POSEIDON_CHECK on a ROUNDS unit; a row index beyond the concatenation; T above 2^32; the usable and tail
 * refusals of kzg_rows_commit_derived; the handle refusals of kzg_rows_open.  After any error the context keeps serving.
 * OUT OF SCOPE: generating constants (the Grain LFSR); other exponents and the inverse S-box; the optimised partial-round form
 * (sparse matrices, pre-folded constants); sponge chaining of one block's output into the next block's input, which is
 * sequential along the column (a Merkle path is a ROW unit, a kzg_rows_commit_fetch and another ROW unit); Poseidon2 (it has
 * its own call, kzg_rows_commit_poseidon2, below).
 * (Sponge chaining and Merkle paths along the column have their own call, kzg_rows_commit_poseidon_chain, below.)
 * SOUNDNESS: nothing here is a proof.  The columns are prover data; the argument is the caller's round gate over the trace
 * columns, in the quotient, under the caller's fixed rc and selector columns.  A zero mismatch count convinces no verifier. */
#define KZG_POSEIDON_ROW    1
#define KZG_POSEIDON_ROUNDS 2
#define KZG_POSEIDON_CHECK  1u               /* flags (ROW): compare with expect, commit nothing */
#define KZG_POSEIDON_IMM    0xffffffffu      /* in[j]: the element is imm_be32[j] */
#define KZG_POSEIDON_NONE   0xffffffffffffffffull   /* out_first_mismatch: no mismatch */
#define KZG_POSEIDON_MIN_T 2
#define KZG_POSEIDON_MAX_T 8
#define KZG_POSEIDON_MAX_FULL 16
#define KZG_POSEIDON_MAX_PARTIAL 128
#define KZG_POSEIDON_MAX_UNITS 8
typedef struct kzg_poseidon_params {
    uint32_t t, full, partial;   /* t in [2, 8]; R_F even in [2, 16]; R_P in [0, 128] */
    const uint8_t* rc_be32;      /* t (full + partial) scalars, round-major */
    const uint8_t* mds_be32;     /* t t scalars, row-major */
} kzg_poseidon_params;
typedef struct kzg_poseidon_unit {
    uint32_t mode;               /* KZG_POSEIDON_ROW or KZG_POSEIDON_ROUNDS */
    uint32_t flags;              /* 0 or KZG_POSEIDON_CHECK */
    uint32_t n_out;              /* ROW: 1 .. t; ROUNDS: t */
    uint32_t period;             /* ROUNDS: P >= R + 1; ROW: 0 */
    uint32_t in[KZG_POSEIDON_MAX_T];       /* [j < t] a row of the concatenated rows of input_handles, or KZG_POSEIDON_IMM */
    uint32_t out[KZG_POSEIDON_MAX_T];      /* [c < n_out] the state element of output column c */
    uint32_t expect[KZG_POSEIDON_MAX_T];   /* [c < n_out] with KZG_POSEIDON_CHECK: the row that column c is compared with */
    uint8_t imm_be32[KZG_POSEIDON_MAX_T][32];   /* [j] the element where in[j] = KZG_POSEIDON_IMM; all zero beside a row */
} kzg_poseidon_unit;
int kzg_rows_commit_poseidon(kzg_ctx* ctx, uint32_t n_input_handles, const uint64_t* input_handles,
                             const kzg_poseidon_params* params, uint32_t n_units, const kzg_poseidon_unit* units,
                             const kzg_derive_opts* opts /* NULL: plain */, uint8_t* out_commitments48 /* n_out * 48 */,
                             uint64_t* out_perms /* n_units */, uint64_t* out_mismatch /* n_units */,
                             uint64_t* out_first_mismatch /* n_units */, uint64_t* out_handle);
/* THE POSEIDON2 PERMUTATION COLUMNS: kzg_rows_commit_poseidon with the Poseidon2 permutation in place of the Hades one: the
 * external layer has no field product and the internal layer has t, so a permutation costs R_F 3 t + R_P (3 + t) products
 * against R_F (3 t + t^2) + R_P (3 + t^2): 408 against 816 at t = 3, (8, 56), and 819 against 4523 at t = 8, (8, 57).  The units
 * are kzg_poseidon_unit with the field meanings, statistics, set, opts and limits of kzg_rows_commit_poseidon; only the
 * parameters and the permutation differ.  The library generates NO constants and ships none: the caller supplies t in {2, 3, 4,
 * 8}, R_F (even, 2 <= R_F <= 16), R_P (0 <= R_P <= 128), the t R_F full-round constants rc_full (round-major: rc_full[rho t + i]
 * for the rho-th FULL round counted over both halves), the R_P partial-round constants rc_partial and the t entries diag, all
 * canonical scalars of 32 big-endian bytes.  The S-box is x -> x^5.  THE EXTERNAL LAYER E:
 *   t = 2, 3   y_i = s_i + sum_j s_j, that is circ(2, 1) and circ(2, 1, 1);
 *   t = 4      y = M4 s, M4 = [[5, 7, 1, 3], [4, 6, 1, 1], [1, 3, 5, 7], [1, 1, 4, 6]];
 *   t = 8      u = (M4 s[0..3], M4 s[4..7]), y_{4k+j} = u_{4k+j} + u_j + u_{4+j}, that is circ(2 M4, M4).
 * THE INTERNAL LAYER I: y_i = diag_i s_i + sum_j s_j, the all-ones matrix plus diag(diag); the published mu_i enter as diag_i =
 * mu_i - 1.  THE PERMUTATION of a state s, R = R_F + R_P:
 *   1. s <- E(s);
 *   2. R_F / 2 full rounds: s_i += rc_full[..] for every i; s_i <- s_i^5 for every i; s <- E(s);
 *   3. R_P partial rounds: s_0 += rc_partial[rho]; s_0 <- s_0^5; s <- I(s);
 *   4. R_F / 2 full rounds as in step 2.
 * KZG_POSEIDON_ROW and its check are kzg_rows_commit_poseidon's.  KZG_POSEIDON_ROUNDS has the period P >= R + 2: block b occupies
 * rows [b P, b P + P); row b P holds the input state, before the first E; row b P + 1 + rho the state BEFORE round rho, so row
 * b P + 1 is E(input) and row b P + 1 + R the output; the remaining rows of the block and the rows behind the last whole block
 * are 0.  The extra row against Poseidon makes every transition a uniform gate: one linear gate from row 0 to row 1, then the
 * round gate.  KZG_E_ARG with a message that begins "poseidon2: " and names the cause: everything kzg_rows_commit_poseidon
 * refuses, and t outside {2, 3, 4, 8}; a null rc_full, rc_partial (with R_P > 0) or diag; a constant at or above r; a period below
 * R + 2.  (The lengths of the three lists are the caller's promise here; the Python layers check them.)
 * OUT OF SCOPE: generating constants and published instance tables; t = 12 .. 24; exponents other than 5; Poseidon2 in
 * kzg_rows_commit_poseidon_chain (sponges and Merkle paths); t lanes per block for traces; any change to the Poseidon kernels.
 * SOUNDNESS: as for kzg_rows_commit_poseidon, nothing here is a proof. */
typedef struct kzg_poseidon2_params {
    uint32_t t, full, partial;      /* t in {2, 3, 4, 8}; R_F even in [2, 16]; R_P in [0, 128] */
    const uint8_t* rc_full_be32;    /* t * full scalars: [rho * t + i] for element i of the rho-th FULL round over both halves */
    const uint8_t* rc_partial_be32; /* `partial` scalars, [rho] for partial round rho; may be NULL when partial = 0 */
    const uint8_t* diag_be32;       /* t scalars, [i] = diag_i: the internal layer is the all-ones matrix plus diag(diag) */
} kzg_poseidon2_params;
#define KZG_POSEIDON2_WIDTHS 0x11cu   /* bit t is set for an allowed width: 2, 3, 4, 8 */
#define KZG_POSEIDON2_MAX_FULL 16
#define KZG_POSEIDON2_MAX_PARTIAL 128
#define KZG_POSEIDON2_MAX_UNITS 8
int kzg_rows_commit_poseidon2(kzg_ctx* ctx, uint32_t n_input_handles, const uint64_t* input_handles,
                              const kzg_poseidon2_params* params, uint32_t n_units, const kzg_poseidon_unit* units,
                              const kzg_derive_opts* opts /* NULL: plain */, uint8_t* out_commitments48 /* n_out * 48 */,
                              uint64_t* out_perms /* n_units */, uint64_t* out_mismatch /* n_units */,
                              uint64_t* out_first_mismatch /* n_units */, uint64_t* out_handle);
/* THE POSEIDON SPONGE AND MERKLE-PATH CHAINS: a set built FROM sets, the two uses of the hash chip that kzg_rows_commit_poseidon
 * leaves out because one block's input depends on the block before through the permutation: a sponge over a message longer than
 * the rate, and a Merkle path.  params is kzg_poseidon_params exactly as kzg_rows_commit_poseidon reads and checks it (t in
 * [2, 8], R_F even, R_P <= 128, the caller's rc and M, S-box x^5, the plain Hades schedule; NO constants are generated).  The
 * concatenated rows of the input_handles sets are the source columns.  A call has 1 <= n_units <= KZG_POSEIDON_CHAIN_MAX_UNITS
 * units that share params.  A SLOT is a source row, or KZG_POSEIDON_IMM: then the value is the slot's imm_be32 on every row,
 * canonical; imm_be32 is all zero beside a row.  With n = opts->usable, or T in the plain layout, every unit is a CHAIN OVER
 * BLOCKS of P = period rows: block b = 0 .. floor(n / P) - 1 occupies rows [b P, b P + P); a block cut by n is not started and
 * its rows are 0.  Block b STARTS A SEGMENT when b = 0, when start is KZG_POSEIDON_CHAIN_ABSENT, or when the start cell at row
 * b P is not zero; otherwise it CONTINUES block b - 1, whose output is out_prev.
 *   KZG_POSEIDON_CHAIN_SPONGE  in[j], j < t, is the slot of state element j.  A starting block's state is (in_0[b P], ..,
 *                              in_{t-1}[b P]), as a ROUNDS unit reads it.  A continuing block's state is state_j = out_prev_j +
 *                              in_j[b P] mod r where in[j] is a row and state_j = out_prev_j where it is an immediate: a tag or
 *                              capacity immediate enters once per message; a continuing block whose rows hold zeros squeezes.
 *                              With start absent the unit IS kzg_rows_commit_poseidon's ROUNDS unit, byte for byte
 *   KZG_POSEIDON_CHAIN_PATH    t >= 3, the arity is a = t - 1.  in[0] is the slot `cap` of state element 0, in[1] the slot `leaf`,
 *                              in[2 + k], k < t - 2, the ROW of sibling k.  State elements 1 .. a are the children: the child at
 *                              position p is cur, the other a - 1 children are the sibling cells of row b P in their order; p is
 *                              the cell of row `pos` at row b P read as a WHOLE canonical integer: a cell at or above a is
 *                              position 0 and is counted once per block in out_bad_pos[u], the smallest such row in
 *                              out_first_bad_pos[u] (2^32 + 1 is bad, not position 1); cur is the leaf cell on a starting block
 *                              and out_prev[digest] on a continuing one.  cap, leaf, the siblings and pos are read at the rows
 *                              b P only
 * layout (a unit that commits): KZG_POSEIDON_CHAIN_TRACE needs P >= R + 1 and commits t columns laid out as a ROUNDS unit lays
 * them out (n_out = t, out[j] = j): row b P + rho holds the state before round rho (row b P the arranged state), row b P + R the
 * output.  KZG_POSEIDON_CHAIN_FLAT takes any P >= 1 and commits the 1 <= n_out <= 2 t distinct columns out[c] names:
 * KZG_POSEIDON_CHAIN_COL_IN + j is element j of the arranged state, KZG_POSEIDON_CHAIN_COL_OUT + j element j of the output, both at
 * row b P only; flat with P = 1 is the one-row-per-level Merkle chip that looks its hashes up in a Poseidon table.  Rows of a
 * block that hold nothing are 0.  With the flag KZG_POSEIDON_CHAIN_CHECK (either mode; layout = 0, n_out = 0) the unit commits
 * NOTHING: at the LAST block of each segment out[digest] is compared with the cell of row `expect` at that block's first row --
 * does every path reach its root, is every message's hash the claimed one -- out_mismatch[u] counts the segments that differ and
 * out_first_mismatch[u] is the smallest such row, or KZG_POSEIDON_NONE.  digest < t is needed by a PATH unit and by a check and
 * is KZG_POSEIDON_CHAIN_ABSENT elsewhere.  out_blocks[u] = floor(n / P), out_segments[u] the blocks that started a segment.
 * All committed columns of a call form ONE new set of the same worker and length, in unit order: out_commitments48[c] equals
 * kzg_rows_commit(i, n_out, these rows, T, 1, ..)[c] byte for byte.  A call of checks alone creates no set (*out_handle = 0,
 * out_commitments48 may be null), reserves nothing and runs no inverse transform and no MSM.  A call reads at most
 * KZG_MAX_BATCH_OPEN distinct rows and commits at most KZG_MAX_BATCH_OPEN.  opts: as for kzg_rows_commit_poseidon, NO closing
 * row.  ONE kernel launch computes every unit, one lane per block; the lane of a segment's first block walks the segment.  A
 * SEGMENT IS SERIAL: it costs its length times one permutation's latency (at t = 3, (8, 57): 0.5 ms measured on one long
 * segment, 1.5 to 1.9 ms in calls of many short ones) whatever the number of segments up to the device's lanes, so
 * a depth-32 path is some 50 ms and ONE message over a whole 2^20-row column at P = 128 took 4.5 s: correct, and slow,
 * like the chains of kzg_rows_commit_sha256 and kzg_rows_commit_keccak.
 * KZG_E_ARG with a message that begins "poseidon_chain: " and names the cause: everything kzg_rows_commit_poseidon refuses about
 * params; n_units outside [1, 4]; an unknown mode, flag or layout; a field the mode does not take (pos on a SPONGE); t = 2 with
 * PATH; an immediate among the siblings, pos, start or expect; digest at or above t, missing where needed, given where not; a
 * TRACE period at or below R, a period of 0; an unknown or repeated column id, n_out = 0 on a FLAT unit; layout or n_out beside
 * KZG_POSEIDON_CHAIN_CHECK; a 17th distinct input row; more than 16 output rows; a row index beyond the concatenation; an
 * immediate at or above r or not zero beside a row; the usable and tail refusals of kzg_rows_commit_derived; the handle refusals
 * of kzg_rows_open.  All but the last four are checked on the host before a lane is taken.
 * OUT OF SCOPE: t cooperating lanes per segment (the follow-up already listed for traces); t above 8, arity-8 trees included;
 * Poseidon2; padding and domain-tag conventions (immediates and the message cells are the caller's); building whole trees level
 * by level (ROW units of kzg_rows_commit_poseidon plus kzg_rows_commit_fetch); a carry across calls.
 * SOUNDNESS: nothing here is a proof.  The columns are prover data; the argument is the caller's gates. */
#define KZG_POSEIDON_CHAIN_SPONGE 1
#define KZG_POSEIDON_CHAIN_PATH   2
#define KZG_POSEIDON_CHAIN_CHECK  1u               /* flags: compare the digest of every segment with expect, commit nothing */
#define KZG_POSEIDON_CHAIN_TRACE  1
#define KZG_POSEIDON_CHAIN_FLAT   2
#define KZG_POSEIDON_CHAIN_ABSENT 0xffffffffu      /* start, pos, digest, expect: none */
#define KZG_POSEIDON_CHAIN_COL_IN  0               /* out[c] (FLAT): + j: element j of the arranged state */
#define KZG_POSEIDON_CHAIN_COL_OUT 8               /* out[c] (FLAT): + j: element j of the block's output */
#define KZG_POSEIDON_CHAIN_MAX_UNITS 4
typedef struct kzg_poseidon_chain_unit {
    uint32_t mode;               /* KZG_POSEIDON_CHAIN_SPONGE or KZG_POSEIDON_CHAIN_PATH */
    uint32_t flags;              /* 0 or KZG_POSEIDON_CHAIN_CHECK */
    uint32_t layout;             /* KZG_POSEIDON_CHAIN_TRACE or KZG_POSEIDON_CHAIN_FLAT; 0 with KZG_POSEIDON_CHAIN_CHECK */
    uint32_t period;             /* P >= 1; TRACE: P >= R + 1 */
    uint32_t start;              /* the row of the start column, or KZG_POSEIDON_CHAIN_ABSENT: every block starts a segment */
    uint32_t pos;                /* PATH: the row of the position column; SPONGE: KZG_POSEIDON_CHAIN_ABSENT */
    uint32_t digest;             /* PATH, CHECK: a state index below t; else KZG_POSEIDON_CHAIN_ABSENT */
    uint32_t expect;             /* CHECK: the row the digest is compared with; else KZG_POSEIDON_CHAIN_ABSENT */
    uint32_t n_out;              /* TRACE: t; FLAT: 1 .. 2 t; CHECK: 0 */
    uint32_t reserved;           /* 0 */
    uint32_t in[KZG_POSEIDON_MAX_T];        /* SPONGE: [j < t] the slot of element j; PATH: cap, leaf, then t - 2 sibling rows */
    uint32_t out[2 * KZG_POSEIDON_MAX_T];   /* [c < n_out] TRACE: c; FLAT: a column id KZG_POSEIDON_CHAIN_COL_IN / _OUT + j, j < t */
    uint8_t imm_be32[KZG_POSEIDON_MAX_T][32];   /* [j] the value where in[j] = KZG_POSEIDON_IMM; all zero beside a row */
} kzg_poseidon_chain_unit;
int kzg_rows_commit_poseidon_chain(kzg_ctx* ctx, uint32_t n_input_handles, const uint64_t* input_handles,
                                   const kzg_poseidon_params* params, uint32_t n_units, const kzg_poseidon_chain_unit* units,
                                   const kzg_derive_opts* opts /* NULL: plain */, uint8_t* out_commitments48 /* n_out * 48 */,
                                   uint64_t* out_blocks /* n_units */, uint64_t* out_segments /* n_units */,
                                   uint64_t* out_bad_pos /* n_units */, uint64_t* out_first_bad_pos /* n_units */,
                                   uint64_t* out_mismatch /* n_units */, uint64_t* out_first_mismatch /* n_units */,
                                   uint64_t* out_handle);
/* THE SHA-256 COMPRESSION COLUMNS: a set built FROM sets, the columns of the bit-oriented hash chip -- Merkle nodes over 32-byte
 * digests, Bitcoin and Ethereum precompile traces, beacon-chain roots.  A round is no polynomial expression (kzg_rows_commit_expr)
 * and depends non-linearly on the four rows before it (kzg_rows_commit_recurrence); composed from kzg_rows_commit_alu it takes
 * more than a hundred calls per column.  There are NO parameters: the 64 round constants K and the standard initial value of
 * FIPS 180-4 are built in.  ALL VALUES ARE 32-BIT WORDS.  A source cell is read as its canonical integer and reduced to its low
 * 32 bits; a cell at or above 2^32 is reduced, never refused, counted once per cell in out_counts[u], and the smallest row of
 * such a cell is out_first[u] (KZG_SHA256_NONE: none): the convention of kzg_rows_commit_int.  Output cells are the words as
 * kzg_rows_commit_int stores them.  The concatenated rows of the input_handles sets (as in kzg_rows_open) are the source
 * columns.  A call has 1 <= n_units <= KZG_SHA256_MAX_UNITS units.  A SLOT is a source row, or KZG_SHA256_IMM: then the word is
 * the slot's immediate on every row, neither read nor counted; the immediate is 0 beside a row.  One row may serve several
 * slots; a unit of immediates alone is legal.  With n = opts->usable, or T in the plain layout:
 *   KZG_SHA256_ROW     for every row t' < n ONE compression of the block msg[0 .. 15] from the chaining value state[0 .. 7] (with
 *                      KZG_SHA256_STD_IV: from the standard initial value; then every state entry is KZG_SHA256_IMM with the
 *                      immediate 0); output column c < n_out holds word out[c] of the new chaining value, feed-forward
 *                      included; 1 <= n_out <= 8, the out[c] distinct and below 8.  With KZG_SHA256_CHECK the unit commits
 *                      NOTHING: expect[c] is the source row that column c is compared with, out_mismatch[u] the number of rows
 *                      t' < n where some expected cell differs from the computed word and out_first_mismatch[u] the smallest
 *                      such row, or KZG_SHA256_NONE.  A 2-to-1 hash of 32-byte nodes is two calls: the first with
 *                      KZG_SHA256_STD_IV and 16 rows, the second with state = the first call's eight output rows and msg = the
 *                      16 padding words as immediates
 *   KZG_SHA256_ROUNDS  the round trace, which is what a prover commits, with the period P = period >= KZG_SHA256_MIN_PERIOD:
 *                      block b = 0 .. floor(n / P) - 1 occupies rows [b P, b P + P); a block cut by n is not started.  msg[0]
 *                      is the row of the message column, start the row of the start column or KZG_SHA256_ABSENT; out[c] < 12,
 *                      distinct, names the column (KZG_SHA256_COL_*) of output column c, 1 <= n_out <= 12.  With W, A, E the
 *                      three main columns of a block, rows counted from the block's first, and H its incoming chaining value:
 *                        rows j = 0 .. 3       A[j] = H[3 - j], E[j] = H[7 - j]: the working variables d, c, b, a and h, g, f, e
 *                        rows q = 4 + t, t < 64  W[q] = W_t: for t < 16 the msg cell at that same row, else sigma1(W[q - 2]) + W[q - 7]
 *                                              + sigma0(W[q - 15]) + W[q - 16] mod 2^32; with (a, b, c, d) = A[q - 1 .. q - 4] and
 *                                              (e, f, g, h) = E[q - 1 .. q - 4]: T1 = h + Sigma1(e) + Ch(e, f, g) + K_t + W[q], T2 =
 *                                              Sigma0(a) + Maj(a, b, c), A[q] = T1 + T2 and E[q] = d + T1 mod 2^32
 *                        rows 68 + j, j < 4    the feed-forward A[68 + j] = A[j] + A[64 + j], E[68 + j] = E[j] + E[64 + j] mod 2^32;
 *                                              the outgoing chaining value is (A[71], A[70], A[69], A[68], E[71], .., E[68])
 *                        rows 72 .. P - 1, and the rows floor(n / P) P .. n - 1: 0 in every column
 *                      so that every gate relates a row to the rows at rotations -1 .. -16.  The columns: W, A, E on all block
 *                      rows (W is 0 outside the rows q); CW the carry floor(. / 2^32) of the schedule sum (rows q, t >= 16); CA
 *                      the carry of T1 + T2 summed in full (rows q) and of the A feed-forward (rows 68 + j); CE the carry of d
 *                      + T1 summed in full (rows q) and of the E feed-forward; SIG0, SIG1 = sigma0(W[q - 15]), sigma1(W[q - 2])
 *                      (rows q, t >= 16); SUM0, MAJ = Sigma0(A[q - 1]), Maj(A[q - 1], A[q - 2], A[q - 3]) and SUM1, CH =
 *                      Sigma1(E[q - 1]), Ch(E[q - 1], E[q - 2], E[q - 3]) (rows q).  A column is 0 on every row not listed for
 *                      it; the carries are at most 3 / 6 / 5.  CHAINING: block b starts a message when b = 0, when start is
 *                      absent, or when the start cell at row b P is not zero (reduced like every cell); its H is then the
 *                      standard initial value (KZG_SHA256_STD_IV) or state_imm[0 .. 7]; else H is the outgoing chaining
 *                      value of block b - 1, so that rows 0 .. 3 repeat rows 68 .. 71 of the block before.  Start cells are
 *                      read at the rows b P of existing blocks only, msg cells at the rows b P + 4 .. b P + 19 only.
 *                      Every state entry is KZG_SHA256_IMM; msg[1 .. 15] and msg_imm are 0; KZG_SHA256_CHECK is refused
 * out_blocks[u] is the number of compressions unit u ran: n for a ROW unit, floor(n / P) for a ROUNDS unit; out_messages[u] the
 * blocks that started a message (0 on a ROW unit); out_mismatch[u] = 0 and out_first_mismatch[u] = KZG_SHA256_NONE on a unit
 * that commits.  All committed columns of a call form ONE new set of the same worker and length, in the order of units, then
 * of out: out_commitments48[c] equals kzg_rows_commit(i, n_out, these rows, T, 1, ..)[c] byte for byte, and *out_handle opens,
 * evaluates, combines, releases, goes stale and counts against KZG_MAX_ROW_SETS like any other.  A call made of checks alone
 * creates no set (*out_handle = 0, out_commitments48 may be null), runs no inverse transform and no MSM.  ONE kernel launch
 * computes every unit; nothing row-sized crosses the host link.  A call reads at most KZG_MAX_BATCH_OPEN distinct rows and
 * commits at most KZG_MAX_BATCH_OPEN.  opts (NULL: plain layout) is kzg_derive_opts as kzg_rows_commit_derived reads it: source
 * rows t' >= usable are never read, compared or counted, output row usable + s of committed column c takes tail_be32[c * (T -
 * usable) + s], there is NO closing row.  Handle lists, worker, T, staleness and threads follow kzg_rows_commit_expr.  KZG_E_ARG
 * with a message that begins "sha256:" and names the cause: n_units outside its range; an unknown mode or flag;
 * KZG_SHA256_CHECK on a ROUNDS unit; a period below 72 (not 0 on a ROW unit); n_out outside its range, an out index at or above
 * 8 (a column id at or above 12) or a repeated one; a state entry, immediate, msg entry or start the mode does not take; more
 * than KZG_MAX_BATCH_OPEN output rows or distinct input rows; a row index beyond the concatenation; T above 2^32; the usable
 * and tail refusals of kzg_rows_commit_derived; the handle refusals of kzg_rows_open.  (An immediate or initial-value word at
 * or above 2^32 does not fit the struct; the Python layer refuses it.)  All but the last five are checked on the host before a
 * lane is taken.  After any error the context keeps serving and no set or buffer leaks.
 * OUT OF SCOPE: padding, and packing bytes into words (compose with kzg_rows_commit_alu / kzg_rows_commit_expr); bit columns
 * and spread-table forms of the words (kzg_rows_commit_derived's limbs and the lookups cover them); SHA-512, Keccak, Blake
 * (Keccak-f[1600] has its own call, kzg_rows_commit_keccak); periods below 72; more than one start convention.  A single message that fills the whole column runs on one lane of the
 * device: correct, and slow.
 * SOUNDNESS: nothing here is a proof.  The columns are prover data; the argument is the caller's gates over these columns plus
 * the range lookups of words and carries.  A zero mismatch count convinces no verifier. */
#define KZG_SHA256_ROW    1
#define KZG_SHA256_ROUNDS 2
#define KZG_SHA256_CHECK  1u               /* flags (ROW): compare with expect, commit nothing */
#define KZG_SHA256_STD_IV 2u               /* flags: the chaining value (ROW) / a message's first one (ROUNDS) is the standard one */
#define KZG_SHA256_IMM    0xffffffffu      /* a slot: the word is the slot's immediate */
#define KZG_SHA256_ABSENT 0xffffffffu      /* start (ROUNDS): every block starts a message */
#define KZG_SHA256_NONE   0xffffffffffffffffull   /* out_first, out_first_mismatch: none */
#define KZG_SHA256_MAX_UNITS 4
#define KZG_SHA256_MIN_PERIOD 72
#define KZG_SHA256_N_COLS 12
#define KZG_SHA256_COL_W 0
#define KZG_SHA256_COL_A 1
#define KZG_SHA256_COL_E 2
#define KZG_SHA256_COL_CW 3
#define KZG_SHA256_COL_CA 4
#define KZG_SHA256_COL_CE 5
#define KZG_SHA256_COL_SIG0 6
#define KZG_SHA256_COL_SIG1 7
#define KZG_SHA256_COL_SUM0 8
#define KZG_SHA256_COL_MAJ 9
#define KZG_SHA256_COL_SUM1 10
#define KZG_SHA256_COL_CH 11
typedef struct kzg_sha256_unit {
    uint32_t mode;               /* KZG_SHA256_ROW or KZG_SHA256_ROUNDS */
    uint32_t flags;              /* a combination of KZG_SHA256_CHECK (ROW) and KZG_SHA256_STD_IV */
    uint32_t n_out;              /* ROW: 1 .. 8; ROUNDS: 1 .. 12 */
    uint32_t period;             /* ROUNDS: P >= 72; ROW: 0 */
    uint32_t start;              /* ROUNDS: the row of the start column, or KZG_SHA256_ABSENT; ROW: KZG_SHA256_ABSENT */
    uint32_t state[8];           /* ROW: [j] the slot of chaining word j; ROUNDS: KZG_SHA256_IMM */
    uint32_t state_imm[8];       /* [j] the word where state[j] = KZG_SHA256_IMM; 0 beside a row and with KZG_SHA256_STD_IV */
    uint32_t msg[16];            /* ROW: [j] the slot of block word j; ROUNDS: msg[0] the row of the message column, the rest 0 */
    uint32_t msg_imm[16];        /* ROW: [j] the word where msg[j] = KZG_SHA256_IMM; 0 beside a row; ROUNDS: 0 */
    uint32_t out[12];            /* [c < n_out] ROW: the chaining word of output column c; ROUNDS: its KZG_SHA256_COL_* */
    uint32_t expect[8];          /* [c < n_out] with KZG_SHA256_CHECK: the row that column c is compared with */
} kzg_sha256_unit;
int kzg_rows_commit_sha256(kzg_ctx* ctx, uint32_t n_input_handles, const uint64_t* input_handles, uint32_t n_units,
                           const kzg_sha256_unit* units, const kzg_derive_opts* opts /* NULL: plain */,
                           uint8_t* out_commitments48 /* n_out * 48 */, uint64_t* out_blocks /* n_units */,
                           uint64_t* out_messages /* n_units */, uint64_t* out_counts /* n_units */,
                           uint64_t* out_first /* n_units */, uint64_t* out_mismatch /* n_units */,
                           uint64_t* out_first_mismatch /* n_units */, uint64_t* out_handle);
/* THE KECCAK-F[1600] PERMUTATION COLUMNS: a set built FROM sets, the columns of the Keccak chip -- storage and account tries, code
 * hashes, the KECCAK256 opcode, SHA-3 and SHAKE.  A round is no polynomial expression (kzg_rows_commit_expr), it is not affine
 * (kzg_rows_commit_recurrence) and it is no 32-bit compression (kzg_rows_commit_sha256); composed from kzg_rows_commit_alu it
 * takes several hundred calls per block.  There are NO parameters: the 24 round constants RC and the rotation offsets r[x][y] of
 * FIPS 202 are built in.  ALL VALUES ARE 64-BIT LANES.  A source cell is read as its canonical integer and reduced to its low
 * 64 bits; a cell at or above 2^64 is reduced, never refused, counted once per cell in out_counts[u], and the smallest row of
 * such a cell is out_first[u] (KZG_KECCAK_NONE: none): the convention of kzg_rows_commit_int.  Output cells are the lanes as
 * kzg_rows_commit_int stores a 64-bit word.  Lane (x, y) of a state has the flat index x + 5 y, the lane order of FIPS 202.  The
 * library deals in integers only; byte order is the caller's: a lane is the little-endian word of 8 message bytes.  The
 * concatenated rows of the input_handles sets (as in kzg_rows_open) are the source columns.  A call has 1 <= n_units <=
 * KZG_KECCAK_MAX_UNITS units.  A SLOT is a source row, or KZG_KECCAK_IMM: then the lane is the slot's immediate on every row,
 * neither read nor counted; the immediate is 0 beside a row.  One row may serve several slots.  With n = opts->usable, or T in
 * the plain layout:
 *   KZG_KECCAK_ROW     for every row t' < n ONE permutation Keccak-f[1600] of the state in[0 .. 24]; output column c < n_out holds
 *                      lane out[c] of the result; 1 <= n_out <= KZG_KECCAK_MAX_OUT, the out[c] distinct and below 25.  A call
 *                      reads at most KZG_MAX_BATCH_OPEN distinct rows, so at least 9 slots are immediates: the shape of hashing
 *                      a short message.  Keccak-256 of two 32-byte nodes is 8 rows, the immediate 0x01 in lane 8, 2^63 in lane
 *                      16, zeros in the capacity, out = 0, 1, 2, 3: ONE call.  With KZG_KECCAK_CHECK the unit commits NOTHING:
 *                      expect[c] is the source row that column c is compared with, out_mismatch[u] the number of rows t' < n
 *                      where some expected cell differs from the computed lane and out_first_mismatch[u] the smallest such
 *                      row, or KZG_KECCAK_NONE.  period and rate are 0, start is KZG_KECCAK_ABSENT
 *   KZG_KECCAK_ROUNDS  the round trace, which is what a prover commits, with the period P = period >= KZG_KECCAK_MIN_PERIOD and
 *                      the rate 1 <= rate <= 24 lanes (17: Keccak-256 and SHA3-256, 9: SHA3-512, 21: SHAKE128): block b = 0 ..
 *                      floor(n / P) - 1 occupies rows [b P, b P + P); a block cut by n is not started.  in[0 .. 4] are the rows
 *                      of the five message columns (in[5 .. 24] and every immediate are 0), start the row of the start column
 *                      or KZG_KECCAK_ABSENT; out[c] < 25, distinct, names the column (KZG_KECCAK_COL_*) of output column c.  Rows
 *                      are counted from the block's first.  With S the block's incoming state, the absorbed state is A_0[x][y]
 *                      = S[x][y] XOR m, m the cell of row in[x] at block row y (reduced and counted) where x + 5 y < rate, else
 *                      0: that cell is then neither read nor counted.
 *                        rows 5 q + y, q < 24, y < 5   round q, plane y: a_x = A[x][y], the state before round q; p_x = A[x][0] ^
 *                                                      .. ^ A[x][y], the running column parity, whose value at y = 4 is C[x];
 *                                                      d_x = D[x] = C[x - 1] ^ rotl(C[x + 1], 1), repeated on the five rows of
 *                                                      the round; t_x = rotl(A[x][y] ^ D[x], r[x][y]): theta and rho at the
 *                                                      source position; b_x = B[x][y], the lane after pi: B[y'][(2 x' + 3 y')
 *                                                      mod 5] = t of (x', y')
 *                        rows 120 + y, y < 5           the outgoing state in the a columns; p, d, t and b are 0
 *                        rows 125 .. P - 1, and the rows floor(n / P) P .. n - 1: 0 in every column
 *                      so that chi and iota are row-local: a_x at row + 5 equals b_x ^ (~b_(x + 1) & b_(x + 2)), XOR RC[q] where
 *                      x = y = 0.  CHAINING: block b starts a message when b = 0, when start is absent, or when the start cell
 *                      at row b P is not zero (reduced like every cell); its S is then all zero; else S is the outgoing state
 *                      of block b - 1.  Start cells are read at the rows b P of existing blocks only.  KZG_KECCAK_CHECK is
 *                      refused.  Padding, domain suffixes and squeezing beyond one block are the caller's
 * out_perms[u] is the number of permutations unit u ran: n for a ROW unit, floor(n / P) for a ROUNDS unit; out_messages[u] the
 * blocks that started a message (0 on a ROW unit); out_mismatch[u] = 0 and out_first_mismatch[u] = KZG_KECCAK_NONE on a unit
 * that commits.  All committed columns of a call form ONE new set of the same worker and length, in the order of units, then
 * of out: out_commitments48[c] equals kzg_rows_commit(i, n_out, these rows, T, 1, ..)[c] byte for byte, and *out_handle opens,
 * evaluates, combines, releases, goes stale and counts against KZG_MAX_ROW_SETS like any other.  A call made of checks alone
 * creates no set (*out_handle = 0, out_commitments48 may be null), runs no inverse transform and no MSM.  ONE kernel launch
 * computes every unit; nothing row-sized crosses the host link.  A call reads at most KZG_MAX_BATCH_OPEN distinct rows and
 * commits at most KZG_MAX_BATCH_OPEN; more columns of a trace take a second unit or call.  opts, handle lists, worker, T,
 * staleness and threads: as for kzg_rows_commit_sha256.  KZG_E_ARG with a message that begins "keccak:" and names the cause:
 * n_units outside its range; an unknown mode or flag; KZG_KECCAK_CHECK on a ROUNDS unit; a period below 125 (not 0 on a ROW
 * unit); a rate outside 1 .. 24 (not 0 on a ROW unit); n_out outside its range, a lane index or column id at or above 25 or a
 * repeated one; an immediate, in entry or start the mode does not take; more than KZG_MAX_BATCH_OPEN output rows or distinct
 * input rows; a row index beyond the concatenation; T above 2^32; the usable and tail refusals of kzg_rows_commit_derived; the
 * handle refusals of kzg_rows_open.  (An immediate at or above 2^64 does not fit the struct; the Python layer refuses it.)  All
 * but the last five are checked on the host before a lane is taken.  After any error the context keeps serving and no set or
 * buffer leaks.
 * OUT OF SCOPE: padding and byte packing; bit columns and spread-table forms of the lanes (kzg_rows_commit_derived's limbs and
 * the lookups cover them); Keccak-f[800] and smaller widths; squeezing more than one block; typed inputs.  A ROUNDS unit runs
 * one lane of the device per message: a single message that fills the whole column is correct, and slow.
 * SOUNDNESS: nothing here is a proof.  The columns are prover data; the argument is the caller's gates over these columns plus
 * the range lookups of the lanes.  A zero mismatch count convinces no verifier. */
#define KZG_KECCAK_ROW    1
#define KZG_KECCAK_ROUNDS 2
#define KZG_KECCAK_CHECK  1u               /* flags (ROW): compare with expect, commit nothing */
#define KZG_KECCAK_IMM    0xffffffffu      /* a slot: the lane is the slot's immediate */
#define KZG_KECCAK_ABSENT 0xffffffffu      /* start (ROUNDS): every block starts a message */
#define KZG_KECCAK_NONE   0xffffffffffffffffull   /* out_first, out_first_mismatch: none */
#define KZG_KECCAK_MAX_UNITS 4
#define KZG_KECCAK_MIN_PERIOD 125
#define KZG_KECCAK_MAX_OUT 16
#define KZG_KECCAK_N_COLS 25
#define KZG_KECCAK_COL_A 0                 /* a0 .. a4: KZG_KECCAK_COL_A + x, and so for the four below */
#define KZG_KECCAK_COL_P 5
#define KZG_KECCAK_COL_D 10
#define KZG_KECCAK_COL_T 15
#define KZG_KECCAK_COL_B 20
typedef struct kzg_keccak_unit {
    uint32_t mode;               /* KZG_KECCAK_ROW or KZG_KECCAK_ROUNDS */
    uint32_t flags;              /* 0 or KZG_KECCAK_CHECK (ROW) */
    uint32_t n_out;              /* 1 .. KZG_KECCAK_MAX_OUT */
    uint32_t period;             /* ROUNDS: P >= 125; ROW: 0 */
    uint32_t rate;               /* ROUNDS: 1 .. 24 lanes; ROW: 0 */
    uint32_t start;              /* ROUNDS: the row of the start column, or KZG_KECCAK_ABSENT; ROW: KZG_KECCAK_ABSENT */
    uint64_t imm[25];            /* ROW: [j] the lane where in[j] = KZG_KECCAK_IMM; 0 beside a row; ROUNDS: 0 */
    uint32_t in[25];             /* ROW: [j] the slot of state lane j = x + 5 y; ROUNDS: in[x < 5] the row of message column x, the rest 0 */
    uint32_t out[16];            /* [c < n_out] ROW: the lane of output column c; ROUNDS: its KZG_KECCAK_COL_* */
    uint32_t expect[16];         /* [c < n_out] with KZG_KECCAK_CHECK: the row that column c is compared with */
} kzg_keccak_unit;
int kzg_rows_commit_keccak(kzg_ctx* ctx, uint32_t n_input_handles, const uint64_t* input_handles, uint32_t n_units,
                           const kzg_keccak_unit* units, const kzg_derive_opts* opts /* NULL: plain */,
                           uint8_t* out_commitments48 /* n_out * 48 */, uint64_t* out_perms /* n_units */,
                           uint64_t* out_messages /* n_units */, uint64_t* out_counts /* n_units */,
                           uint64_t* out_first /* n_units */, uint64_t* out_mismatch /* n_units */,
                           uint64_t* out_first_mismatch /* n_units */, uint64_t* out_handle);
/* THE NON-NATIVE ELLIPTIC-CURVE COLUMNS: a set built FROM sets, the columns of the chip that does curve arithmetic over a FOREIGN
 * field -- ecrecover and ECDSA over secp256k1, the bn254 precompiles, P-256.  The slope of a point addition is a modular
 * division, which kzg_rows_commit_wide leaves out; a scalar multiplication is a chain whose accumulator feeds the next row
 * non-linearly, which neither kzg_rows_commit_expr (no dependence from row to row) nor kzg_rows_commit_recurrence (affine)
 * expresses.  VALUES follow kzg_rows_commit_wide: a wide value is L = curve->limbs consecutive limb rows of b = curve->bits bits,
 * little-endian, 1 <= b <= 64, 1 <= L <= KZG_EC_MAX_LIMBS, W = b L <= 256; a cell is read as its canonical integer and reduced
 * to its low b bits.  THE CURVE is one per call: p = curve->p (four little-endian 64-bit words), ODD, 3 <= p < 2^W, not
 * necessarily prime, and a = curve->a < p, the coefficient of y^2 = x^3 + a x + c; c is never needed and not taken.  An operand
 * at or above p is reduced mod p, never refused.  A row with a limb at or above 2^b or an operand at or above p is counted ONCE
 * per unit in out_counts[u], the smallest such row is out_first[u] (KZG_EC_NONE: none).  The concatenated rows of the
 * input_handles sets (as in kzg_rows_open) are the source columns; an operand is named by its FIRST row and runs over L rows;
 * one row may serve several operands.  A call has 1 <= n_units <= KZG_EC_MAX_UNITS units.  With n = opts->usable, or T in the
 * plain layout, and every row t' < n on its own:
 *   KZG_EC_DIV    r = a b^-1 mod p, L output rows; in[0] = a, in[1] = b, or with KZG_EC_IMM_B in[1] = KZG_EC_ABSENT and b = imm
 *                 on every row (below 2^W; reduced mod p like a row, not counted).  Where gcd(b mod p, p) != 1 (b = 0 mod p
 *                 included) r = 0 and the row is counted in out_singular[u], the smallest such row in out_first_singular[u].
 *                 cols is KZG_EC_R.  The caller's gate is kzg_rows_commit_wide's MULMOD / CARRY of r b = a + q p.
 *   KZG_EC_ADD    in[0 .. 3] = x1, y1, x2, y2, all reduced mod p.  x1 != x2: lambda = (y2 - y1) / (x2 - x1); x1 = x2, y1 = y2 and
 *                 gcd(2 y1, p) = 1: lambda = (3 x1^2 + a) / (2 y1), the doubling (name the same rows twice to double a
 *                 column); any other row -- opposite points, a point of order two, a denominator without an inverse under a
 *                 composite p -- is EXCEPTIONAL: lambda = x3 = y3 = 0, counted in out_singular[u] / out_first_singular[u].
 *                 x3 = lambda^2 - x1 - x2, y3 = lambda (x1 - x3) - y1.  cols picks among KZG_EC_LAM, KZG_EC_X3, KZG_EC_Y3; the
 *                 output rows come in that order, L rows each.  There is no point at infinity and no on-curve check: the unit
 *                 is arithmetic on pairs of integers.
 *   KZG_EC_CHECK  (a flag on DIV and ADD) the unit commits NOTHING: expect[k] is the first row of the L rows that name k of cols
 *                 is compared with (DIV: expect[0]; ADD: expect[0 .. 2] for lambda, x3, y3; KZG_EC_ABSENT beside a name that is
 *                 not in cols); out_mismatch[u] is the number of rows t' < n where some expected cell differs from the computed
 *                 limb, out_first_mismatch[u] the smallest such row.
 *   KZG_EC_CHAIN  the accumulator trace of a double-and-add or of a multi-scalar sum: in[0] = px, in[1] = py, op the row of the
 *                 op-code column (ONE row, compared as a whole integer); cols picks among KZG_EC_AX, KZG_EC_AY, KZG_EC_LAM, in
 *                 that order.  The accumulator is a pair of integers mod p, (0, 0) before row 0.  Row t holds the accumulator
 *                 BEFORE the step in ax, ay and the step's lambda in lam (0 where there is none); then op[t] acts: 0 hold; 1
 *                 load, acc <- (px[t], py[t]); 2 acc <- acc + (px[t], py[t]) by the rule of ADD, the doubling included; 3 acc
 *                 <- 2 acc; any other code holds and is counted in out_unknown[u] / out_first_unknown[u].  An exceptional step
 *                 leaves acc = (0, 0) and is counted in out_singular[u].  px and py are neither read nor counted on rows whose
 *                 op is 0, 3 or unknown.  A SEGMENT begins at row 0 and at every load; out_segments[u] is their number.  The
 *                 chain stops at n; there is no closing row: a caller that wants the last result ends on a hold row.
 *                 KZG_EC_CHECK is refused.
 * Statistics a mode does not have are 0 and KZG_EC_NONE.  All committed rows of a call form ONE new set of the same worker and
 * length, in the order of units, then of names, then of limbs: out_commitments48[c] equals kzg_rows_commit(i, n_out, these rows,
 * T, 1, ..)[c] byte for byte, and *out_handle opens, evaluates, combines, releases, goes stale and counts against
 * KZG_MAX_ROW_SETS like any other.  A call made of checks alone creates no set (*out_handle = 0, out_commitments48 may be
 * null), runs no inverse transform and no MSM.  ONE kernel launch computes every unit; nothing row-sized crosses the host link.
 * A call reads at most KZG_MAX_BATCH_OPEN distinct rows (two points of L = 4 are 16) and commits at most KZG_MAX_BATCH_OPEN.
 * opts, handle lists, worker, T, staleness and threads: as for kzg_rows_commit_keccak.  KZG_E_ARG with a message that begins
 * "ec:" and names the cause: n_units outside its range; b, L or W outside their ranges; p even, below 3 or at or above 2^W;
 * a >= p; an unknown mode or flag, KZG_EC_CHECK on a CHAIN unit, KZG_EC_IMM_B beside a mode other than DIV; cols empty or with a
 * name the mode does not have; an operand, op, expect entry or immediate the mode does not take, or a missing one; an
 * immediate at or above 2^W; an operand run that reaches beyond the concatenation; more than KZG_MAX_BATCH_OPEN output rows
 * or distinct input rows; T above 2^32; the usable and tail refusals of kzg_rows_commit_derived; the handle refusals of
 * kzg_rows_open.  All but the last four are checked on the host before a lane is taken.  After any error the context keeps
 * serving and no set or buffer leaks.
 * OUT OF SCOPE: L > 4 (BLS12-381's Fp); Edwards and Montgomery forms; projective coordinates; the point at infinity; an
 * on-curve check; subtraction or negation ops; per-row moduli; an even modulus; the quotient and carry columns of the gates
 * (kzg_rows_commit_wide over these outputs gives them).  A CHAIN unit runs one lane of the device per segment: one segment that
 * fills the whole column is correct, and slow.  (Twisted Edwards curves over the scalar field ITSELF -- Jubjub,
 * Bandersnatch -- are not foreign and have their own call, kzg_rows_commit_edwards, whose chain walks in projective coordinates
 * with no inversion per step.)
 * SOUNDNESS: nothing here is a proof.  The columns are prover data; the argument is the caller's MULMOD / CARRY gates over
 * lambda, x3 and y3 (lambda (x2 - x1) = y2 - y1, and so on, mod p) plus the range lookups of every limb.  Zero counts convince
 * no verifier. */
#define KZG_EC_DIV   1
#define KZG_EC_ADD   2
#define KZG_EC_CHAIN 3
#define KZG_EC_CHECK 1u                /* flags (DIV, ADD): compare with expect, commit nothing */
#define KZG_EC_IMM_B 2u                /* flags (DIV): operand b is imm */
#define KZG_EC_R     1u                /* cols (DIV) */
#define KZG_EC_LAM   1u                /* cols (ADD): lambda, x3, y3 */
#define KZG_EC_X3    2u
#define KZG_EC_Y3    4u
#define KZG_EC_AX    1u                /* cols (CHAIN): ax, ay, lam */
#define KZG_EC_AY    2u
#define KZG_EC_CLAM  4u
#define KZG_EC_ABSENT 0xffffffffu      /* an operand, op or expect entry the unit does not have */
#define KZG_EC_NONE   0xffffffffffffffffull   /* out_first*: none */
#define KZG_EC_MAX_UNITS 4
#define KZG_EC_MAX_LIMBS 4
typedef struct kzg_ec_curve {
    uint32_t bits;               /* b: 1 .. 64 */
    uint32_t limbs;              /* L: 1 .. KZG_EC_MAX_LIMBS, b L <= 256 */
    uint64_t p[4];               /* the modulus, little-endian words: odd, 3 <= p < 2^(b L) */
    uint64_t a[4];               /* the coefficient a < p */
} kzg_ec_curve;
typedef struct kzg_ec_unit {
    uint32_t mode;               /* KZG_EC_DIV, KZG_EC_ADD or KZG_EC_CHAIN */
    uint32_t flags;              /* KZG_EC_CHECK, KZG_EC_IMM_B */
    uint32_t cols;               /* the names that are committed (or compared), a mask of the mode's KZG_EC_* names */
    uint32_t op;                 /* CHAIN: the row of the op-code column; else KZG_EC_ABSENT */
    uint32_t in[4];              /* first rows.  DIV: a, b; ADD: x1, y1, x2, y2; CHAIN: px, py; KZG_EC_ABSENT beyond */
    uint32_t expect[3];          /* with KZG_EC_CHECK: [k] the first row name k is compared with; else KZG_EC_ABSENT */
    uint32_t reserved;           /* 0 */
    uint64_t imm[4];             /* with KZG_EC_IMM_B: b, little-endian words; else 0 */
} kzg_ec_unit;
int kzg_rows_commit_ec(kzg_ctx* ctx, uint32_t n_input_handles, const uint64_t* input_handles, const kzg_ec_curve* curve,
                       uint32_t n_units, const kzg_ec_unit* units, const kzg_derive_opts* opts /* NULL: plain */,
                       uint8_t* out_commitments48 /* n_out * 48 */, uint64_t* out_counts /* n_units */,
                       uint64_t* out_first /* n_units */, uint64_t* out_singular /* n_units */,
                       uint64_t* out_first_singular /* n_units */, uint64_t* out_mismatch /* n_units */,
                       uint64_t* out_first_mismatch /* n_units */, uint64_t* out_unknown /* n_units */,
                       uint64_t* out_first_unknown /* n_units */, uint64_t* out_segments /* n_units */, uint64_t* out_handle);
/* THE NATIVE TWISTED-EDWARDS COLUMNS: a set built FROM sets, the columns of the chip that does curve arithmetic on a twisted
 * Edwards curve defined over the scalar field Fr ITSELF -- Jubjub (RedJubjub signatures and Pedersen hashes of Zcash Sapling),
 * Bandersnatch (the Pedersen vector commitments of Ethereum's Verkle tries).  A coordinate is ONE cell of ONE resident row, read
 * as the field element it is: no limbs, no range counts.  The accumulator trace of a scalar multiplication depends on the row
 * before it non-linearly, which neither kzg_rows_commit_expr (no dependence from row to row) nor kzg_rows_commit_recurrence
 * (affine) expresses, and kzg_rows_commit_ec works on limbs over a foreign field with no Edwards form.  THE CURVE is one per
 * call: A x^2 + y^2 = 1 + D x^2 y^2 with A = curve->a_be32 and D = curve->d_be32, canonical scalars, A != 0, D != 0, A != D.  The
 * library generates no curve and ships no constant.  THE LAW is arithmetic on pairs of field elements, with no on-curve check;
 * the neutral element is (0, 1).  With tau = D x1 x2 y1 y2:
 *     x3 = (x1 y2 + y1 x2) / (1 + tau)          y3 = (y1 y2 - A x1 x2) / (1 - tau)
 * and the doubling is this same formula with both operands equal (a dedicated doubling that substitutes the curve equation
 * differs on off-curve pairs and is not used).  A row or step with tau = 1 or tau = -1 is EXCEPTIONAL.  The concatenated rows of
 * the input_handles sets (as in kzg_rows_open) are the source columns.  An operand slot in[w] is a row index, or
 * KZG_EDWARDS_IMM: then the operand is imm_be32[w] on every row (canonical; a constant point, a fixed base, the neutral
 * element); imm_be32[w] is 0 beside a row.  A call has 1 <= n_units <= KZG_EDWARDS_MAX_UNITS units.  With n = opts->usable, or
 * T in the plain layout:
 *   KZG_EDWARDS_ADD    in[0 .. 3] = x1, y1, x2, y2; one addition per row t' < n.  cols picks among KZG_EDWARDS_X3 and
 *                      KZG_EDWARDS_Y3; out_order[0 .. n_cols) lists the picked names (0: x3, 1: y3) in the order of their output
 *                      rows (KZG_EDWARDS_ABSENT beyond).  An exceptional row writes x3 = y3 = 0, is counted in out_singular[u],
 *                      and the smallest such row is out_first_singular[u] (KZG_EDWARDS_NONE: none).  Name the same rows twice to
 *                      double a column.
 *   KZG_EDWARDS_CHECK  (a flag on ADD) the unit commits NOTHING: expect[k] is the row that name k of cols is compared with
 *                      (KZG_EDWARDS_ABSENT beside a name that is not in cols; out_order is all KZG_EDWARDS_ABSENT);
 *                      out_mismatch[u] is the number of rows t' < n where an expected cell differs from the computed one (an
 *                      exceptional row computes 0), out_first_mismatch[u] the smallest such row.  No inversion runs: the
 *                      device compares expect (1 +- tau) with the numerator.
 *   KZG_EDWARDS_CHAIN  the accumulator trace of a double-and-add or of a multi-scalar sum: in[0] = px, in[1] = py, op the row of
 *                      the op-code column (compared as a whole 255-bit integer); cols picks among KZG_EDWARDS_AX and
 *                      KZG_EDWARDS_AY, out_order as above (0: ax, 1: ay).  The accumulator is (0, 1) before row 0.  Row t holds
 *                      the accumulator BEFORE the step; then op[t] acts: 0 hold; 1 load, acc <- (px[t], py[t]); 2 acc <- acc +
 *                      (px[t], py[t]); 3 acc <- acc + acc; 4 acc <- acc + (-px[t], py[t]); any other value (2^32 + 2 is one)
 *                      holds and is counted in out_unknown[u] / out_first_unknown[u].  An exceptional step leaves acc = (0, 1)
 *                      and is counted in out_singular[u].  px and py are not read where op is 0, 3 or unknown.  A SEGMENT
 *                      begins at row 0 and at every load; out_segments[u] is their number.  The chain stops at n; there is no
 *                      closing row.  KZG_EDWARDS_CHECK is refused.
 * Statistics a mode does not have are 0 and KZG_EDWARDS_NONE.  All committed rows of a call form ONE new set of the same worker
 * and length, in the order of units, then of out_order: out_commitments48[c] equals kzg_rows_commit(i, n_out, these rows, T, 1,
 * ..)[c] byte for byte, and *out_handle opens, evaluates, combines, releases, goes stale and counts against KZG_MAX_ROW_SETS
 * like any other.  A call made of checks alone creates no set (*out_handle = 0, out_commitments48 may be null), runs no inverse
 * transform and no MSM.  ON THE DEVICE: one launch computes every unit WITHOUT a field inversion -- an ADD unit leaves the
 * numerators (x1 y2 + y1 x2)(1 - tau), (y1 y2 - A x1 x2)(1 + tau) and the denominator 1 - tau^2; a CHAIN unit walks its
 * segments in projective coordinates (X : Y : Z) with the unified mixed addition and leaves X, Y and Z per row -- then ONE
 * batched inversion over the denominators of every unit, then one launch that multiplies through.  Nothing row-sized crosses
 * the host link.  A call reads at most KZG_MAX_BATCH_OPEN distinct rows and commits at most KZG_MAX_BATCH_OPEN.  opts, handle
 * lists, worker, T, staleness and threads: as for kzg_rows_commit_ec.  KZG_E_ARG with a message that begins "edwards:" and
 * names the cause: n_units outside its range; A, D or an immediate not canonical; A = 0, D = 0 or A = D; an unknown mode or
 * flag, KZG_EDWARDS_CHECK on a CHAIN unit; cols empty or with a name the mode does not have; an out_order that is not the
 * picked names once each; an operand, op or expect entry the mode does not take, or a missing one; a non-zero immediate beside
 * a row; a row beyond the concatenation; more than KZG_MAX_BATCH_OPEN output rows or distinct input rows; T above 2^32; the
 * usable and tail refusals of kzg_rows_commit_derived; the handle refusals of kzg_rows_open.  All but the last four are
 * checked on the host before a lane is taken.  After any error the context keeps serving and no set or buffer leaks.
 * OUT OF SCOPE: Montgomery and short-Weierstrass forms over Fr; a per-row scalar multiplication (a chain segment gives it, with
 * its trace); a helper column for tau (an expression column: kzg_rows_commit_expr); on-curve and subgroup checks; windowed or
 * signed-digit op-codes beyond 4; parallelism inside one segment: a CHAIN unit runs one lane of the device per segment.
 * SOUNDNESS: nothing here is a proof.  The columns are prover data; the argument is the caller's two addition gates, x3 (1 +
 * D x1 x2 y1 y2) = x1 y2 + y1 x2 and y3 (1 - D x1 x2 y1 y2) = y1 y2 - A x1 x2, under the op-code's selector.  Zero counts
 * convince no verifier. */
#define KZG_EDWARDS_ADD   1
#define KZG_EDWARDS_CHAIN 2
#define KZG_EDWARDS_CHECK 1u                /* flags (ADD): compare with expect, commit nothing */
#define KZG_EDWARDS_X3    1u                /* cols (ADD): x3, y3 */
#define KZG_EDWARDS_Y3    2u
#define KZG_EDWARDS_AX    1u                /* cols (CHAIN): ax, ay */
#define KZG_EDWARDS_AY    2u
#define KZG_EDWARDS_IMM    0xfffffffeu      /* in[w]: the operand is imm_be32[w] */
#define KZG_EDWARDS_ABSENT 0xffffffffu      /* an operand, op, expect or out_order entry the unit does not have */
#define KZG_EDWARDS_NONE   0xffffffffffffffffull   /* out_first*: none */
#define KZG_EDWARDS_MAX_UNITS 4
typedef struct kzg_edwards_curve {
    uint8_t a_be32[32];          /* A: canonical, not 0 */
    uint8_t d_be32[32];          /* D: canonical, not 0, not A */
} kzg_edwards_curve;
typedef struct kzg_edwards_unit {
    uint32_t mode;               /* KZG_EDWARDS_ADD or KZG_EDWARDS_CHAIN */
    uint32_t flags;              /* KZG_EDWARDS_CHECK */
    uint32_t cols;               /* the names that are committed (or compared), a mask of the mode's KZG_EDWARDS_* names */
    uint32_t op;                 /* CHAIN: the row of the op-code column; else KZG_EDWARDS_ABSENT */
    uint32_t in[4];              /* rows or KZG_EDWARDS_IMM.  ADD: x1, y1, x2, y2; CHAIN: px, py; KZG_EDWARDS_ABSENT beyond */
    uint32_t expect[2];          /* with KZG_EDWARDS_CHECK: [k] the row name k is compared with; else KZG_EDWARDS_ABSENT */
    uint32_t out_order[2];       /* the picked names (0 or 1) in the order of their output rows; KZG_EDWARDS_ABSENT beyond */
    uint8_t imm_be32[4][32];     /* [w]: the operand where in[w] is KZG_EDWARDS_IMM; else 0 */
} kzg_edwards_unit;
int kzg_rows_commit_edwards(kzg_ctx* ctx, uint32_t n_input_handles, const uint64_t* input_handles,
                            const kzg_edwards_curve* curve, uint32_t n_units, const kzg_edwards_unit* units,
                            const kzg_derive_opts* opts /* NULL: plain */, uint8_t* out_commitments48 /* n_out * 48 */,
                            uint64_t* out_singular /* n_units */, uint64_t* out_first_singular /* n_units */,
                            uint64_t* out_mismatch /* n_units */, uint64_t* out_first_mismatch /* n_units */,
                            uint64_t* out_unknown /* n_units */, uint64_t* out_first_unknown /* n_units */,
                            uint64_t* out_segments /* n_units */, uint64_t* out_handle);
/* THE QUOTIENT WITH LOOKUP SELECTORS: kzg_rows_commit_quotient_zk and kzg_rows_quotient_part for lookups that are enabled on
 * some rows only.  selectors->selector_rows holds L = lookup->n_lookups entries, each a row index into the call's concatenated
 * rows (the caller's fixed column q_l, the row that kzg_rows_commit_multiplicities_sel / _lookup_sum_sel read) or
 * KZG_NO_SELECTOR (the constant 1); one row may serve several lookups.  The selector becomes the numerator of its fraction, at
 * no cost in degree.  With D_0 = beta + Tb, D_l = beta + F_l for lookup l = 1 .. L and q_l that lookup's selector:
 *   LK1 = (S(w X) - S(X)) prod_{l=0..L} D_l  -  [ sum_{l=1..L} q_l prod_{l' != l, l'=0..L} D_l'  -  m prod_{l=1..L} D_l ]
 * q_l prod_{l' != l} D_l' has L + 1 factors, still below the L + 2 of the first product: L <= E - 1 (E - 2 with an active
 * column) and the piece counts stay as they are.  D_l stands on EVERY row, enabled or not.  A selector row is extended once
 * like any row the call names and shares its extended vector if it is also a gate factor or the active column; a selected
 * lookup costs one more 32-byte load and one more product per point.  selectors == NULL, or every entry KZG_NO_SELECTOR, IS
 * the existing call (kzg_rows_commit_quotient_zk / kzg_rows_quotient_part), byte for byte and kernel for kernel; an all-ones
 * selector row gives the same bytes.  Errors beyond the existing call's (all KZG_E_ARG): selectors != NULL with lookup ==
 * NULL; a null selector_rows; a selector row index >= n.  Everything else -- handle rules, the accumulator, thread safety, a
 * racing release or SRS load, "after any error the context keeps serving" -- is the existing call's. */
typedef struct kzg_quotient_selectors {
    const uint32_t* selector_rows;   /* L; row index or KZG_NO_SELECTOR */
} kzg_quotient_selectors;
int kzg_rows_commit_quotient_sel(kzg_ctx* ctx, uint32_t n_handles, const uint64_t* handles, const kzg_quotient_terms* gate,
                                 const kzg_quotient_perm* perm /* NULL: none */,
                                 const kzg_quotient_lookup* lookup /* NULL: none */,
                                 const kzg_quotient_selectors* selectors /* NULL: kzg_rows_commit_quotient_zk */,
                                 const kzg_quotient_active* active /* NULL: none */, uint32_t ext_log, uint32_t n_pieces,
                                 uint8_t* out_commitments48 /* n_pieces * 48 */, uint64_t* out_handle);
int kzg_rows_quotient_part_sel(kzg_ctx* ctx, uint32_t n_handles, const uint64_t* handles, const kzg_quotient_terms* gate,
                               const kzg_quotient_perm* perm, const kzg_quotient_link* link, const kzg_quotient_lookup* lookup,
                               const kzg_quotient_selectors* selectors /* NULL: kzg_rows_quotient_part */,
                               const kzg_quotient_active* active, uint32_t ext_log, const uint8_t* scale_be32 /* NULL: 1 */,
                               uint64_t* inout_acc);
/* The UNCHANGED reference miner makes two calls per request with the same row -- worker_commit(i, poly), then
 * worker_open(i, poly, x) (neurons/miner.py:56-61).  These forms take a 128-bit content tag identifying the row's bytes
 * (the host codec computes it while decoding the text); the coefficient vectors of the last four rows stay on the
 * device, and a call whose (tag, T, evaluation_form) is cached skips the INTT and keeps the row's upload off its critical
 * path.  A miss behaves exactly like kzg_commit / kzg_open and leaves its own coefficients behind.  Results are
 * identical either way, whatever the tags: a tag is a HINT -- on a hit the library uploads row_be32 beside the request
 * and compares it bit for bit with the row the slot was filled from; two different rows under one tag each get their
 * own answer (the colliding slot is dropped and the call recomputed), so a fast non-cryptographic tag is safe. */
int kzg_commit_cached(kzg_ctx* ctx, uint32_t i, const uint8_t* row_be32, uint64_t T, int evaluation_form,
                      const uint8_t content_tag[16], uint8_t out_commitment48[48]);
int kzg_open_cached(kzg_ctx* ctx, uint32_t i, const uint8_t* row_be32, uint64_t T, int evaluation_form,
                    const uint8_t content_tag[16], const uint8_t alpha_be32[32], uint8_t out_eval32[32],
                    uint8_t out_proof48[48]);
int kzg_row_cache_stats(kzg_ctx* ctx, uint64_t out_hits_misses[2]);
/* plain MSM over resident points [srs_offset, srs_offset+n): the headline kernel (BASELINE.json metric) */
int kzg_msm(kzg_ctx* ctx, const uint8_t* scalars_be32, uint64_t n, uint64_t srs_offset, uint8_t out48[48]);
/* replaces Client.fft(poly, left, inverse)          (reference neurons/validator.py:58-65); in place */
int kzg_ntt(kzg_ctx* ctx, uint8_t* inout_be32, uint64_t n, int inverse);
/* replaces Client.eval(poly, x)                     (reference neurons/validator.py:97-104) */
int kzg_eval(kzg_ctx* ctx, const uint8_t* coeffs_be32, uint64_t n, const uint8_t x_be32[32], uint8_t out_be32[32]);
/* both in one call: y = (NTT / inverse NTT of vals)(x) -- the validator's per-row challenge step
 * eval(fft(poly[i], left=True, inverse=True), alpha) (reference neurons/validator.py:115-118) with the coefficient
 * vector staying on the device */
int kzg_ntt_eval(kzg_ctx* ctx, const uint8_t* vals_be32, uint64_t n, int inverse, const uint8_t x_be32[32],
                 uint8_t out_y32[32]);

/* ---- verification: replaces Client.worker_verify(i, proof, alpha, eval, commitment)
 *      (reference neurons/validator.py:77-86; tests/test_miner.py:101-111).  Host-side pairing check
 *      e(C - y [L_i]_1, [1]_2) == e(pi, [tau_x - alpha]_2): one-off per proof, no GPU involved, so the verifier key is
 *      its own object.  *out_valid = 1 / 0; malformed or off-curve proof / commitment bytes give valid = 0. */
typedef struct kzg_vk kzg_vk;
/* tau_g2: uncompressed G2 x.c1||x.c0||y.c1||y.c0 (4 x 48 B big-endian); li_g1: [L_i(tau_y)]_1 per resident slice */
int kzg_vk_create(const uint8_t tau_g2_be192[192], const uint8_t* li_g1_be96, uint32_t n_slices, kzg_vk** out);
/* synthetic setup with known trapdoor (same tau / s0 as kzg_gen_srs): tests and benches */
int kzg_vk_create_synthetic(const uint8_t tau_be32[32], const uint8_t* s0_be32, uint32_t n_slices, kzg_vk** out);
void kzg_vk_destroy(kzg_vk* vk);
/* serialise: 192 B [tau_x]_2 + 96 B per slice (a `<setup>.vk` file); returns the slice count or a negative status */
int kzg_vk_export(const kzg_vk* vk, uint8_t* out, uint64_t out_len);
int kzg_vk_verify(const kzg_vk* vk, uint32_t i, const uint8_t proof48[48], const uint8_t alpha_be32[32],
                  const uint8_t eval_be32[32], const uint8_t commitment48[48], int* out_valid);
/* Every row of a validator step in ONE pairing check (the rows share alpha: neurons/validator.py:106-120).  Random
 * 128-bit weights r_i (getrandom) fold the n checks into two Miller loops on sum r_i (C_i - y_i L_i) and sum r_i pi_i;
 * the per-row work (decompression, G1 membership, three scalar multiplications) runs on `threads` host threads.
 * *out_all_valid = 1 only when every row is valid (an invalid one slips through with probability 2^-128); on 0 call
 * kzg_vk_verify row by row to find which.  idx: the worker index of each row. */
int kzg_vk_verify_batch(const kzg_vk* vk, uint32_t n, const uint32_t* idx, const uint8_t* proofs48,
                        const uint8_t alpha_be32[32], const uint8_t* evals_be32, const uint8_t* commitments48, int threads,
                        int* out_all_valid);
/* One batched opening (kzg_commit_open_batch) of k rows of slice i:
 *   e(sum_j gamma^j C_j - (sum_j gamma^j y_j) [L_i]_1, [1]_2) == e(pi, [tau_x - alpha]_2).
 * Same rules as kzg_vk_verify: malformed, off-curve or non-G1 commitment / proof bytes give *out_valid = 0 (not an error);
 * k = 0, k > KZG_MAX_BATCH_OPEN or i outside the key -> KZG_E_ARG; alpha, gamma or an evaluation >= r -> KZG_E_SCALAR. */
int kzg_vk_verify_open_batch(const kzg_vk* vk, uint32_t i, uint32_t k, const uint8_t* commitments48,
                             const uint8_t* evals_be32, const uint8_t alpha_be32[32], const uint8_t gamma_be32[32],
                             const uint8_t proof48[48], int* out_valid);
/* One multi-point opening (kzg_commit_open_multi) of k rows of slice i: for every point p
 *   e(A_p, [1]_2) == e(pi_p, [tau_x - alpha_p]_2),  A_p = sum_t gamma_p^t C_{j_t} - (sum_t gamma_p^t y_{j_t,p}) [L_i]_1,
 * folded with fresh 128-bit random weights r_p (getrandom, as in kzg_vk_verify_batch) into two Miller loops:
 *   e(sum_p r_p (A_p + alpha_p pi_p), [1]_2) * e(-sum_p r_p pi_p, [tau_x]_2) == 1.
 * evals_be32 in the layout kzg_commit_open_multi writes.  Malformed, off-curve or non-G1 commitment / proof bytes give
 * *out_valid = 0 (not an error); k, m or a mask outside the rules of kzg_commit_open_multi, or i outside the key -> KZG_E_ARG;
 * an alpha_p, gamma_p or evaluation >= r -> KZG_E_SCALAR. */
int kzg_vk_verify_open_multi(const kzg_vk* vk, uint32_t i, uint32_t k, const uint8_t* commitments48, uint32_t m,
                             const uint8_t* points_be32, const uint32_t* masks, const uint8_t* gammas_be32,
                             const uint8_t* evals_be32, const uint8_t* proofs48, int* out_valid);
/* One caller-weighted opening (kzg_rows_open_lincomb) of k rows of slice i, every point folded with random 128-bit weights
 * into two Miller loops as in kzg_vk_verify_open_multi:
 *   e(sum_j lambda_{p,j} C_j - v_p [L_i]_1, [1]_2) == e(pi_p, [tau_x - alpha_p]_2)  for every p.
 * coeffs_be32: m x k, point-major, as kzg_rows_open_lincomb takes them.  Malformed, off-curve or non-G1 commitment / proof
 * bytes give *out_valid = 0 (not an error); k = 0, k > KZG_MAX_BATCH_OPEN, m = 0, m > KZG_MAX_OPEN_POINTS, a point whose
 * coefficients are all zero or i outside the key -> KZG_E_ARG; an alpha_p, coefficient or value >= r -> KZG_E_SCALAR. */
int kzg_vk_verify_open_lincomb(const kzg_vk* vk, uint32_t i, uint32_t k, const uint8_t* commitments48, uint32_t m,
                               const uint8_t* points_be32, const uint8_t* coeffs_be32, const uint8_t* values_be32,
                               const uint8_t* proofs48, int* out_valid);
/* One SHPLONK opening (kzg_rows_commit_shplonk + kzg_rows_open_lincomb at u) of k rows of slice i at m points.  evals32: the
 * evaluations y_{j,p} in the point-major layout of kzg_rows_eval for the same points and masks.  The host computes r_j(u) by
 * Lagrange interpolation over S_j, from them v and the lambda of round B, and runs the check of kzg_vk_verify_open_lincomb on
 * the k + 1 commitments (C_0 .. C_{k-1}, W) at the one point u with value v and proof pi: two pairings whatever m is.
 * Malformed, off-curve or non-G1 commitment / W / proof bytes and a well-formed but false proof give *out_ok = 0 (not an
 * error).  The argument checks of kzg_rows_commit_shplonk (each KZG_E_ARG), u equal to one of the points or i outside the
 * key -> KZG_E_ARG; an evaluation or u >= r -> KZG_E_SCALAR. */
int kzg_vk_verify_open_shplonk(const kzg_vk* vk, uint32_t i, uint32_t k, const uint8_t* commitments48 /* k*48 */, uint32_t m,
                               const uint8_t* points_be32, const uint32_t* masks, const uint8_t* coeffs_be32 /* k*32 */,
                               const uint8_t* evals32 /* kzg_rows_eval's point-major layout */,
                               const uint8_t w48[48], const uint8_t u_be32[32], const uint8_t proof48[48], int* out_ok);

/* ---- multi-GPU: each rank reduces its SRS shard to ONE partial sum; the 192-byte partials are exchanged by
 *      the caller (RCCL all_gather over xGMI in zkp_subnet_amd.distributed) and summed on any rank. */
/* (A partial is a projective XYZZ representative: two runs over the same input may return different bytes for the
 *  same group element.  Only kzg_g1_sum's 48-byte output is canonical.) */
int kzg_msm_partial(kzg_ctx* ctx, const uint8_t* scalars_be32, uint64_t n, uint64_t srs_offset,
                    uint8_t out_xyzz192[192]);
int kzg_g1_sum(kzg_ctx* ctx, const uint8_t* partials_xyzz192, uint32_t count, uint8_t out48[48]);
/* Pianist master aggregation: sum of `count` 48-byte compressed G1 points (the worker rows' commitments,
 * sum_i commit_i = commitment of the bivariate polynomial; reference neurons/validator.py:196-198, README.md:38).
 * Inputs are decompressed on the GPU (one Fp square root each) and checked for membership in G1 (the prime-order
 * subgroup: they come from untrusted miners); malformed / off-curve / out-of-subgroup input -> KZG_E_POINT. */
int kzg_g1_sum_compressed(kzg_ctx* ctx, const uint8_t* points_c48, uint32_t count, uint8_t out48[48]);
/* Device-pointer forms for the collective path: the partial is written into / the gathered partials are read from the
 * CALLER's device memory (the tensors of an RCCL all_gather), so a step makes no host round trip for them.
 * kzg_msm_partial_resident_dev returns after its stream has drained (dev_out is complete); the caller must have
 * completed the collective (stream synchronised) before kzg_g1_sum_dev. */
int kzg_msm_partial_resident_dev(kzg_ctx* ctx, int slot, uint64_t n, uint64_t srs_offset, void* dev_out_xyzz192);
int kzg_g1_sum_dev(kzg_ctx* ctx, const void* dev_partials_xyzz192, uint32_t count, uint8_t out48[48]);
/* The same step chained through streams, one host synchronisation per MSM.  _begin queues the MSM of this rank's SRS
 * segment on a free lane, writes its 192-byte partial to dev_out_xyzz192 and makes `consumer_stream` (a hipStream_t: the
 * stream the collective is enqueued on, e.g. torch's current stream) wait for it ON THE DEVICE; it returns a ticket
 * without blocking.  After the all_gather has been enqueued on that stream, _finish makes the lane wait for
 * `producer_stream` in turn, sums the `count` gathered partials on the lane and returns the compressed point.
 * (the exchange is 192 B per rank, latency-bound -- host round trips around it are what it costs.) */
int kzg_msm_sharded_begin(kzg_ctx* ctx, int slot, uint64_t n, uint64_t srs_offset, void* dev_out_xyzz192,
                          void* consumer_stream, int* out_ticket);
int kzg_msm_sharded_finish(kzg_ctx* ctx, int ticket, const void* dev_partials_xyzz192, uint32_t count,
                           void* producer_stream, uint8_t out48[48]);

/* ---- the collective INSIDE the library ("RCCL is used directly from C++"; one process per GPU, rank g
 *      holds SRS segment g).  The only exchange of an SRS-sharded MSM is one ncclAllGather of 192 bytes per rank; these
 *      entry points own the communicator and enqueue that all_gather on the LANE's own stream, between the partial and
 *      the sum: no foreign stream, no event hand-over, one host wait per MSM, no framework underneath (the reference
 *      seam is one client object per process, base/miner.py:73-84).  RCCL is bound at the first kzg_comm_* call
 *      (dlopen of librccl.so.1 -- the copy the process already maps, if any; KZG_RCCL_LIB names another file); without
 *      it these calls fail with KZG_E_COMM and everything else works as before.
 *  kzg_comm_unique_id   ncclGetUniqueId: ONE rank calls it and hands the 128 bytes to every rank by any means it has
 *                       (a file, a socket, torch.distributed's store, MPI): the rendezvous is the caller's.
 *  kzg_comm_init        ncclCommInitRank on the context's device; collective over the `world` ranks (blocks until all
 *                       have called it).  Waits for the lanes to be idle; KZG_E_BUSY while a ticket is out.
 *  kzg_comm_init_bounded the same with a deadline: the rendezvous AND a first checked 192-byte all_gather (which connects the
 *                       transports) run on a helper thread that holds nothing of the context; when the `world` ranks have
 *                       not joined and exchanged within init_timeout_ms (0 = wait for ever = kzg_comm_init) the call returns
 *                       KZG_E_COMM and the context keeps serving -- a peer that never arrives costs one timeout, never a
 *                       wedged context (a helper still blocked inside RCCL's rendezvous is left behind; it owns nothing).
 *  kzg_comm_set_timeout per-call budget in ms for kzg_msm_sharded (0 = wait for ever, the default).  When it expires the
 *                       communicator is ABORTED (ncclCommAbort: the stuck collective leaves the stream), the call and every
 *                       later one return KZG_E_COMM until kzg_comm_destroy + kzg_comm_init -- a dead peer costs one
 *                       timeout, never a parked axon thread.  A call on ANOTHER lane whose collective was in flight under
 *                       the aborted communicator returns KZG_E_COMM too, never a result (checked after its wait).
 *  kzg_comm_info        out[0] rank, out[1] world (0 = no communicator), out[2] RCCL version (e.g. 22707), out[3] 1 if broken.
 *  kzg_comm_selftest    one small all_gather with checked content (rank i sends 192 bytes of value i + 1): run it right
 *                       after kzg_comm_init, before tables are built -- ncclCommInitRank succeeding does not prove that bytes
 *                       move between these ranks.  Collective; honours the timeout.
 *  kzg_msm_sharded      the MSM of this rank's segment (resident scalars in `slot`, points [srs_offset, srs_offset + n)
 *                       of this rank's resident SRS) -> 192-byte partial -> ncclAllGather on the lane's stream -> sum of
 *                       the `world` partials -> 48-byte compressed point, the same on every rank.  Thread-safe like every
 *                       call (each takes a lane); ranks must issue their sharded MSMs in the same order (RCCL's rule for
 *                       collectives on one communicator). */
int kzg_comm_unique_id(uint8_t out_id128[128]);
int kzg_comm_init(kzg_ctx* ctx, const uint8_t unique_id128[128], int rank, int world);
int kzg_comm_init_bounded(kzg_ctx* ctx, const uint8_t unique_id128[128], int rank, int world, int init_timeout_ms);
int kzg_comm_destroy(kzg_ctx* ctx);
int kzg_comm_set_timeout(kzg_ctx* ctx, int timeout_ms);
int kzg_comm_info(kzg_ctx* ctx, int32_t out[4]);
int kzg_comm_selftest(kzg_ctx* ctx);
int kzg_msm_sharded(kzg_ctx* ctx, int slot, uint64_t n, uint64_t srs_offset, uint8_t out48[48]);

/* ---- several GPUs behind ONE handle (SURVEY 8b proposed kzg_create(device_count, device_ids); the reference builds one
 *      prover client per process, base/miner.py:73-84).  One context per GPU inside; host threads only; thread-safe like a
 *      context.  Two layouts, chosen by the load call:
 *  ROWS -- worker index i is served by device_ids[i mod G].  The in-process form of the reference's only distribution scheme:
 *      Pianist rows are independent, one row per miner (neurons/validator.py:194-222).  Nothing is exchanged.
 *  kzg_multi_load_srs_file   every device loads, in parallel, ONLY the slices of the worker indices it serves (i = g, g + G, ...:
 *                            kzg_load_srs_file_slices) -- 1 / G of the file, of the tables and of the start time each
 *  kzg_multi_gen_srs         synthetic SRS: s0_be32_all holds ALL 2^machines_scale slice factors; device g generates and
 *                            holds only the slices of the worker indices it serves
 *  kzg_multi_commit / _open / _commit_open        = kzg_commit / kzg_open / kzg_commit_open on the device of index i
 *  kzg_multi_commit_open_rows   the rows of one challenge fanned out over the devices from host threads (up to four rows per
 *                            device in flight); out_status[k] is row k's own status -- a bad row never costs the others
 *  SEGMENTS -- ONE MSM over all the GPUs of the handle (BASELINE.json configs[3] from behind the one-client seam): a flat SRS of
 *      n_points is cut into G contiguous segments (sizes differ by at most one), segment g resident on device g.
 *  kzg_multi_load_srs_file_segments   device g reads file points [lo_g, lo_g + n_g) only (kzg_load_srs_file_range)
 *  kzg_multi_gen_srs_segments         synthetic: point j = [tau^j] G; s0_be32_per_device[g] = tau^(lo_g) (G x 32 bytes, computed
 *                            by the caller: tests and benches only); kzg_multi_segment reports lo_g and n_g
 *  kzg_multi_msm             sum_j s_j P_(srs_offset + j), j < n: device g computes the partial of its part of the range on its
 *                            own lane (all devices concurrently, scalars uploaded straight to their device), the G 192-byte
 *                            partials come back through the host and are summed once -- no collective, the exchange is G x 192 B.
 *                            Bit-identical to kzg_msm over the same points on one device.
 *  kzg_multi_upload_fr / kzg_multi_msm_resident   the same with the scalars resident in HBM (segment g's scalars in slot
 *                            `slot` of device g): what a serving loop and bench.py time
 *  After a load that failed on ANY device the handle refuses every routed call (KZG_E_ARG) until a load has succeeded on all
 *  of them: the devices that did load already hold the new SRS, so no layout describes the handle in between.
 *  kzg_multi_ctx             the k-th per-GPU context: every other call of this header applies to it */
typedef struct kzg_multi kzg_multi;
int kzg_multi_create(int device_count, const int* device_ids, kzg_multi** out);
void kzg_multi_destroy(kzg_multi* m);
const char* kzg_multi_last_error(kzg_multi* m); /* last failure of the calling thread */
int kzg_multi_count(kzg_multi* m);
kzg_ctx* kzg_multi_ctx(kzg_multi* m, int k);
int kzg_multi_device_of(kzg_multi* m, uint32_t i);
int kzg_multi_load_srs_file(kzg_multi* m, const char* path, int compressed, int scale, int machines_scale);
int kzg_multi_gen_srs(kzg_multi* m, const uint8_t tau_be32[32], const uint8_t* s0_be32_all, int scale, int machines_scale);
int kzg_multi_load_srs_file_segments(kzg_multi* m, const char* path, int compressed, uint64_t n_points);
int kzg_multi_gen_srs_segments(kzg_multi* m, const uint8_t tau_be32[32], const uint8_t* s0_be32_per_device, uint64_t n_points);
int kzg_multi_segment(kzg_multi* m, int g, uint64_t out_first_count[2]);
int kzg_multi_msm(kzg_multi* m, const uint8_t* scalars_be32, uint64_t n, uint64_t srs_offset, uint8_t out48[48]);
int kzg_multi_upload_fr(kzg_multi* m, int slot, const uint8_t* scalars_be32, uint64_t n, uint64_t srs_offset);
int kzg_multi_msm_resident(kzg_multi* m, int slot, uint8_t out48[48]);
int kzg_multi_commit(kzg_multi* m, uint32_t i, const uint8_t* row_be32, uint64_t T, int evaluation_form,
                     uint8_t out_commitment48[48]);
int kzg_multi_open(kzg_multi* m, uint32_t i, const uint8_t* row_be32, uint64_t T, int evaluation_form,
                   const uint8_t alpha_be32[32], uint8_t out_eval32[32], uint8_t out_proof48[48]);
int kzg_multi_commit_open(kzg_multi* m, uint32_t i, const uint8_t* row_be32, uint64_t T, int evaluation_form,
                          const uint8_t alpha_be32[32], uint8_t out_commitment48[48], uint8_t out_eval32[32],
                          uint8_t out_proof48[48]);
int kzg_multi_commit_open_rows(kzg_multi* m, uint32_t n_rows, const uint32_t* indices, const uint8_t* rows_be32, uint64_t T,
                               int evaluation_form, const uint8_t alpha_be32[32], uint8_t* out_commitments48,
                               uint8_t* out_evals32, uint8_t* out_proofs48, int* out_status);
/* kzg_commit_open_batch on the device of worker i (routed like kzg_multi_commit_open) */
int kzg_multi_commit_open_batch(kzg_multi* m, uint32_t i, uint32_t k, const uint8_t* rows_be32, uint64_t T,
                                int evaluation_form, const uint8_t alpha_be32[32], const uint8_t gamma_be32[32],
                                uint8_t* out_commitments48, uint8_t* out_evals32, uint8_t out_proof48[48]);
/* kzg_commit_open_multi on the device of worker i (routed like kzg_multi_commit_open) */
int kzg_multi_commit_open_multi(kzg_multi* mh, uint32_t i, uint32_t k, const uint8_t* rows_be32, uint64_t T,
                                int evaluation_form, uint32_t m, const uint8_t* points_be32, const uint32_t* masks,
                                const uint8_t* gammas_be32, uint8_t* out_commitments48, uint8_t* out_evals32,
                                uint8_t* out_proofs48);
/* committed row sets on the device of worker i (routed like kzg_multi_commit_open): every set named in an open, an
 * evaluation, a lincomb opening or a release must belong to worker i, else KZG_E_ARG */
int kzg_multi_rows_commit(kzg_multi* mh, uint32_t i, uint32_t k, const uint8_t* rows_be32, uint64_t T, int evaluation_form,
                          uint8_t* out_commitments48, uint64_t* out_handle);
int kzg_multi_rows_open(kzg_multi* mh, uint32_t i, uint32_t n_handles, const uint64_t* handles, uint32_t m,
                        const uint8_t* points_be32, const uint32_t* masks, const uint8_t* gammas_be32, uint8_t* out_evals32,
                        uint8_t* out_proofs48);
int kzg_multi_rows_release(kzg_multi* mh, uint32_t i, uint64_t handle);
int kzg_multi_rows_commit_typed(kzg_multi* mh, uint32_t i, uint32_t k, const kzg_col* cols, uint64_t T, int evaluation_form,
                                uint8_t* out_commitments48, uint64_t* out_handle);
int kzg_multi_rows_read(kzg_multi* mh, uint32_t i, uint32_t n_handles, const uint64_t* handles, uint32_t row, uint64_t first,
                        uint64_t count, uint32_t kind, int evaluation_form, void* out, uint64_t out_overflow[2]);
int kzg_multi_rows_eval(kzg_multi* mh, uint32_t i, uint32_t n_handles, const uint64_t* handles, uint32_t m,
                        const uint8_t* points_be32, const uint32_t* masks, uint8_t* out_evals32);
int kzg_multi_rows_open_lincomb(kzg_multi* mh, uint32_t i, uint32_t n_handles, const uint64_t* handles, uint32_t k,
                                uint32_t m, const uint8_t* points_be32, const uint8_t* coeffs_be32, uint8_t* out_values32,
                                uint8_t* out_proofs48);
/* kzg_rows_commit_shplonk on the device of worker i: every set named must belong to worker i, else KZG_E_ARG */
int kzg_multi_rows_commit_shplonk(kzg_multi* mh, uint32_t i, uint32_t n_handles, const uint64_t* handles, uint32_t k, uint32_t m,
                                  const uint8_t* points_be32, const uint32_t* masks, const uint8_t* coeffs_be32,
                                  uint8_t out_commitment48[48], uint64_t* out_handle);
/* kzg_rows_commit_grand_product on the device of worker i: every set named must belong to worker i, else KZG_E_ARG */
int kzg_multi_rows_commit_grand_product(kzg_multi* mh, uint32_t i, uint32_t n_wire_handles, const uint64_t* wire_handles,
                                        uint32_t n_sigma_handles, const uint64_t* sigma_handles, uint32_t k,
                                        const uint8_t* shifts_be32, const uint8_t beta_be32[32], const uint8_t gamma_be32[32],
                                        uint8_t out_commitment48[48], uint8_t out_closing32[32], uint64_t* out_handle);
/* kzg_rows_commit_lookup_sum on the device of worker i: every set named must belong to worker i, else KZG_E_ARG */
int kzg_multi_rows_commit_lookup_sum(kzg_multi* mh, uint32_t i, uint32_t n_input_handles, const uint64_t* input_handles,
                                     uint32_t n_table_handles, const uint64_t* table_handles, uint64_t mult_handle,
                                     uint32_t n_lookups, uint32_t width, const uint8_t theta_be32[32],
                                     const uint8_t beta_be32[32], uint8_t out_commitment48[48], uint8_t out_closing32[32],
                                     uint64_t* out_handle);
/* kzg_rows_commit_multiplicities on the device of worker i: every set named must belong to worker i, else KZG_E_ARG */
int kzg_multi_rows_commit_multiplicities(kzg_multi* mh, uint32_t i, uint32_t n_input_handles, const uint64_t* input_handles,
                                         uint32_t n_table_handles, const uint64_t* table_handles, uint32_t n_lookups,
                                         uint32_t width, uint8_t out_commitment48[48], uint64_t* out_missing,
                                         uint64_t* out_handle);
/* kzg_rows_commit_quotient on the device of worker i: every set named must belong to worker i, else KZG_E_ARG */
int kzg_multi_rows_commit_quotient(kzg_multi* mh, uint32_t i, uint32_t n_handles, const uint64_t* handles,
                                   const kzg_quotient_gate* gate, const kzg_quotient_perm* perm, uint32_t ext_log,
                                   uint32_t n_pieces, uint8_t* out_commitments48, uint64_t* out_handle);
/* kzg_rows_commit_quotient_ext on the device of worker i: every set named must belong to worker i, else KZG_E_ARG */
int kzg_multi_rows_commit_quotient_ext(kzg_multi* mh, uint32_t i, uint32_t n_handles, const uint64_t* handles,
                                       const kzg_quotient_terms* gate, const kzg_quotient_perm* perm,
                                       const kzg_quotient_lookup* lookup, uint32_t ext_log, uint32_t n_pieces,
                                       uint8_t* out_commitments48, uint64_t* out_handle);
/* the kzg_rows_commit_*_zk builders on the device of worker i: every set named must belong to worker i, else KZG_E_ARG */
int kzg_multi_rows_commit_grand_product_zk(kzg_multi* mh, uint32_t i, uint32_t n_wire_handles, const uint64_t* wire_handles,
                                           uint32_t n_sigma_handles, const uint64_t* sigma_handles, uint32_t k,
                                           const uint8_t* shifts_be32, const uint8_t beta_be32[32], const uint8_t gamma_be32[32],
                                           uint64_t usable, const uint8_t* tail_be32, uint8_t out_commitment48[48],
                                           uint8_t out_closing32[32], uint64_t* out_handle);
int kzg_multi_rows_commit_lookup_sum_zk(kzg_multi* mh, uint32_t i, uint32_t n_input_handles, const uint64_t* input_handles,
                                        uint32_t n_table_handles, const uint64_t* table_handles, uint64_t mult_handle,
                                        uint32_t n_lookups, uint32_t width, const uint8_t theta_be32[32],
                                        const uint8_t beta_be32[32], uint64_t usable, const uint8_t* tail_be32,
                                        uint8_t out_commitment48[48], uint8_t out_closing32[32], uint64_t* out_handle);
int kzg_multi_rows_commit_multiplicities_zk(kzg_multi* mh, uint32_t i, uint32_t n_input_handles, const uint64_t* input_handles,
                                            uint32_t n_table_handles, const uint64_t* table_handles, uint32_t n_lookups,
                                            uint32_t width, uint64_t usable, const uint8_t* tail_be32,
                                            uint8_t out_commitment48[48], uint64_t* out_missing, uint64_t* out_handle);
/* the kzg_rows_commit_*_sel builders on the device of worker i: every set named, selector sets included, must belong to worker i */
int kzg_multi_rows_commit_lookup_sum_sel(kzg_multi* mh, uint32_t i, uint32_t n_input_handles, const uint64_t* input_handles,
                                         uint32_t n_table_handles, const uint64_t* table_handles, uint64_t mult_handle,
                                         uint32_t n_sel_handles, const uint64_t* sel_handles, const uint32_t* sel_index,
                                         uint32_t n_lookups, uint32_t width, const uint8_t theta_be32[32],
                                         const uint8_t beta_be32[32], uint64_t usable, const uint8_t* tail_be32,
                                         uint8_t out_commitment48[48], uint8_t out_closing32[32], uint64_t* out_handle);
int kzg_multi_rows_commit_multiplicities_sel(kzg_multi* mh, uint32_t i, uint32_t n_input_handles, const uint64_t* input_handles,
                                             uint32_t n_table_handles, const uint64_t* table_handles, uint32_t n_sel_handles,
                                             const uint64_t* sel_handles, const uint32_t* sel_index, uint32_t n_lookups,
                                             uint32_t width, uint64_t usable, const uint8_t* tail_be32,
                                             uint8_t out_commitment48[48], uint64_t* out_missing, uint64_t* out_handle);
int kzg_multi_rows_commit_quotient_zk(kzg_multi* mh, uint32_t i, uint32_t n_handles, const uint64_t* handles,
                                      const kzg_quotient_terms* gate, const kzg_quotient_perm* perm,
                                      const kzg_quotient_lookup* lookup, const kzg_quotient_active* active, uint32_t ext_log,
                                      uint32_t n_pieces, uint8_t* out_commitments48, uint64_t* out_handle);
int kzg_multi_rows_quotient_part(kzg_multi* mh, uint32_t i, uint32_t n_handles, const uint64_t* handles,
                                 const kzg_quotient_terms* gate, const kzg_quotient_perm* perm, const kzg_quotient_link* link,
                                 const kzg_quotient_lookup* lookup, const kzg_quotient_active* active, uint32_t ext_log,
                                 const uint8_t* scale_be32, uint64_t* inout_acc);
int kzg_multi_rows_commit_quotient_sel(kzg_multi* mh, uint32_t i, uint32_t n_handles, const uint64_t* handles,
                                       const kzg_quotient_terms* gate, const kzg_quotient_perm* perm,
                                       const kzg_quotient_lookup* lookup, const kzg_quotient_selectors* selectors,
                                       const kzg_quotient_active* active, uint32_t ext_log, uint32_t n_pieces,
                                       uint8_t* out_commitments48, uint64_t* out_handle);
int kzg_multi_rows_quotient_part_sel(kzg_multi* mh, uint32_t i, uint32_t n_handles, const uint64_t* handles,
                                     const kzg_quotient_terms* gate, const kzg_quotient_perm* perm, const kzg_quotient_link* link,
                                     const kzg_quotient_lookup* lookup, const kzg_quotient_selectors* selectors,
                                     const kzg_quotient_active* active, uint32_t ext_log, const uint8_t* scale_be32,
                                     uint64_t* inout_acc);
int kzg_multi_rows_quotient_finish(kzg_multi* mh, uint32_t i, uint64_t acc, uint32_t n_pieces, uint8_t* out_commitments48,
                                   uint64_t* out_handle);
int kzg_multi_rows_commit_grand_product_chain(kzg_multi* mh, uint32_t i, uint32_t n_wire_handles, const uint64_t* wire_handles,
                                              uint32_t n_sigma_handles, const uint64_t* sigma_handles, uint32_t k,
                                              const uint8_t* shifts_be32, const uint8_t beta_be32[32],
                                              const uint8_t gamma_be32[32], uint64_t usable, const uint8_t* tail_be32,
                                              const uint8_t start_be32[32], uint8_t out_commitment48[48],
                                              uint8_t out_closing32[32], uint64_t* out_handle);
/* kzg_rows_commit_shuffle on the device of worker i: every set named must belong to worker i, else KZG_E_ARG */
int kzg_multi_rows_commit_shuffle(kzg_multi* mh, uint32_t i, uint32_t n_input_handles, const uint64_t* input_handles,
                                  uint32_t n_shuffle_handles, const uint64_t* shuffle_handles, uint32_t n_groups, uint32_t width,
                                  const uint8_t theta_be32[32], const uint8_t gamma_be32[32], const kzg_shuffle_opts* opts,
                                  uint8_t out_commitment48[48], uint8_t out_closing32[32], uint64_t* out_handle);
/* kzg_rows_commit_sorted on the device of worker i: every set named must belong to worker i, else KZG_E_ARG */
int kzg_multi_rows_commit_sorted(kzg_multi* mh, uint32_t i, uint32_t n_input_handles, const uint64_t* input_handles,
                                 uint32_t width, uint32_t n_keys, const kzg_sorted_opts* opts, uint8_t* out_commitments48,
                                 uint64_t* out_handle);
/* kzg_rows_commit_derived on the device of worker i: every set named must belong to worker i, else KZG_E_ARG */
int kzg_multi_rows_commit_derived(kzg_multi* mh, uint32_t i, uint32_t n_input_handles, const uint64_t* input_handles,
                                  uint32_t n_ops, const kzg_derive_op* ops, const kzg_derive_opts* opts,
                                  uint8_t* out_commitments48, uint64_t* out_counts, uint64_t* out_handle);
/* kzg_rows_commit_expr on the device of worker i: every set named must belong to worker i, else KZG_E_ARG */
int kzg_multi_rows_commit_expr(kzg_multi* mh, uint32_t i, uint32_t n_input_handles, const uint64_t* input_handles,
                               uint32_t n_exprs, const kzg_expr* exprs, const kzg_expr_opts* opts, uint8_t* out_commitments48,
                               uint64_t* out_nonzero, uint64_t* out_first, uint64_t* out_handle);
/* kzg_rows_commit_recurrence on the device of worker i: every set named must belong to worker i, else KZG_E_ARG */
int kzg_multi_rows_commit_recurrence(kzg_multi* mh, uint32_t i, uint32_t n_input_handles, const uint64_t* input_handles,
                                     uint32_t n_recs, const kzg_recurrence* recs, const kzg_recurrence_opts* opts,
                                     uint8_t* out_commitments48, uint8_t* out_closings32, uint64_t* out_handle);
/* kzg_rows_commit_fetch on the device of worker i: every set named must belong to worker i, else KZG_E_ARG */
int kzg_multi_rows_commit_fetch(kzg_multi* mh, uint32_t i, uint32_t n_input_handles, const uint64_t* input_handles,
                                uint32_t n_table_handles, const uint64_t* table_handles, uint32_t n_reads, uint32_t n_keys,
                                uint32_t flags, const kzg_derive_opts* opts, uint8_t* out_commitments48, uint64_t* out_missing,
                                uint64_t* out_first_missing, uint64_t* out_handle);
/* kzg_rows_commit_sigma / kzg_rows_check_copies on the device of worker i: every set named must belong to worker i, else
 * KZG_E_ARG */
int kzg_multi_rows_commit_sigma(kzg_multi* mh, uint32_t i, uint32_t n_label_handles, const uint64_t* label_handles, uint32_t k,
                                const uint8_t* shifts_be32, const kzg_sigma_opts* opts, uint8_t* out_commitments48,
                                uint64_t out_stats[2], uint64_t* out_handle);
int kzg_multi_rows_check_copies(kzg_multi* mh, uint32_t i, uint32_t n_wire_handles, const uint64_t* wire_handles,
                                uint32_t n_label_handles, const uint64_t* label_handles, uint32_t k, const kzg_sigma_opts* opts,
                                uint64_t out[2]);
/* kzg_rows_commit_int on the device of worker i: every set named must belong to worker i, else KZG_E_ARG */
int kzg_multi_rows_commit_int(kzg_multi* mh, uint32_t i, uint32_t n_input_handles, const uint64_t* input_handles, uint32_t n_ops,
                              const kzg_int_op* ops, const kzg_derive_opts* opts, uint8_t* out_commitments48,
                              uint64_t* out_counts, uint64_t* out_first, uint64_t* out_handle);
/* kzg_rows_commit_alu on the device of worker i: every set named must belong to worker i, else KZG_E_ARG */
int kzg_multi_rows_commit_alu(kzg_multi* mh, uint32_t i, uint32_t n_input_handles, const uint64_t* input_handles,
                              uint32_t n_entries, const kzg_alu_entry* program, uint32_t n_units, const kzg_alu_unit* units,
                              const kzg_derive_opts* opts, uint8_t* out_commitments48, uint64_t* out_counts, uint64_t* out_first,
                              uint64_t* out_unknown, uint64_t* out_first_unknown, uint64_t* out_handle);
/* kzg_rows_commit_wide on the device of worker i: every set named must belong to worker i, else KZG_E_ARG */
int kzg_multi_rows_commit_wide(kzg_multi* mh, uint32_t i, uint32_t n_input_handles, const uint64_t* input_handles, uint32_t n_ops,
                               const kzg_wide_op* ops, const kzg_derive_opts* opts, uint8_t* out_commitments48,
                               uint64_t* out_counts, uint64_t* out_first, uint64_t* out_qover, uint64_t* out_first_qover,
                               uint64_t* out_handle);
/* kzg_rows_commit_poseidon_chain on the device of worker i: every set named must belong to worker i, else KZG_E_ARG */
int kzg_multi_rows_commit_poseidon_chain(kzg_multi* mh, uint32_t i, uint32_t n_input_handles, const uint64_t* input_handles,
                                         const kzg_poseidon_params* params, uint32_t n_units,
                                         const kzg_poseidon_chain_unit* units, const kzg_derive_opts* opts,
                                         uint8_t* out_commitments48, uint64_t* out_blocks, uint64_t* out_segments,
                                         uint64_t* out_bad_pos, uint64_t* out_first_bad_pos, uint64_t* out_mismatch,
                                         uint64_t* out_first_mismatch, uint64_t* out_handle);
/* kzg_rows_commit_poseidon on the device of worker i: every set named must belong to worker i, else KZG_E_ARG */
int kzg_multi_rows_commit_poseidon(kzg_multi* mh, uint32_t i, uint32_t n_input_handles, const uint64_t* input_handles,
                                   const kzg_poseidon_params* params, uint32_t n_units, const kzg_poseidon_unit* units,
                                   const kzg_derive_opts* opts, uint8_t* out_commitments48, uint64_t* out_perms,
                                   uint64_t* out_mismatch, uint64_t* out_first_mismatch, uint64_t* out_handle);
/* kzg_rows_commit_poseidon2 on the device of worker i: every set named must belong to worker i, else KZG_E_ARG */
int kzg_multi_rows_commit_poseidon2(kzg_multi* mh, uint32_t i, uint32_t n_input_handles, const uint64_t* input_handles,
                                    const kzg_poseidon2_params* params, uint32_t n_units, const kzg_poseidon_unit* units,
                                    const kzg_derive_opts* opts, uint8_t* out_commitments48, uint64_t* out_perms,
                                    uint64_t* out_mismatch, uint64_t* out_first_mismatch, uint64_t* out_handle);
/* kzg_rows_commit_sha256 on the device of worker i: every set named must belong to worker i, else KZG_E_ARG */
int kzg_multi_rows_commit_sha256(kzg_multi* mh, uint32_t i, uint32_t n_input_handles, const uint64_t* input_handles,
                                 uint32_t n_units, const kzg_sha256_unit* units, const kzg_derive_opts* opts,
                                 uint8_t* out_commitments48, uint64_t* out_blocks, uint64_t* out_messages, uint64_t* out_counts,
                                 uint64_t* out_first, uint64_t* out_mismatch, uint64_t* out_first_mismatch, uint64_t* out_handle);
/* kzg_rows_commit_keccak on the device of worker i: every set named must belong to worker i, else KZG_E_ARG */
int kzg_multi_rows_commit_keccak(kzg_multi* mh, uint32_t i, uint32_t n_input_handles, const uint64_t* input_handles,
                                 uint32_t n_units, const kzg_keccak_unit* units, const kzg_derive_opts* opts,
                                 uint8_t* out_commitments48, uint64_t* out_perms, uint64_t* out_messages, uint64_t* out_counts,
                                 uint64_t* out_first, uint64_t* out_mismatch, uint64_t* out_first_mismatch, uint64_t* out_handle);
/* kzg_rows_commit_ec on the device of worker i: every set named must belong to worker i, else KZG_E_ARG */
int kzg_multi_rows_commit_ec(kzg_multi* mh, uint32_t i, uint32_t n_input_handles, const uint64_t* input_handles,
                             const kzg_ec_curve* curve, uint32_t n_units, const kzg_ec_unit* units, const kzg_derive_opts* opts,
                             uint8_t* out_commitments48, uint64_t* out_counts, uint64_t* out_first, uint64_t* out_singular,
                             uint64_t* out_first_singular, uint64_t* out_mismatch, uint64_t* out_first_mismatch,
                             uint64_t* out_unknown, uint64_t* out_first_unknown, uint64_t* out_segments, uint64_t* out_handle);
/* kzg_rows_commit_edwards on the device of worker i: every set named must belong to worker i, else KZG_E_ARG */
int kzg_multi_rows_commit_edwards(kzg_multi* mh, uint32_t i, uint32_t n_input_handles, const uint64_t* input_handles,
                                  const kzg_edwards_curve* curve, uint32_t n_units, const kzg_edwards_unit* units,
                                  const kzg_derive_opts* opts, uint8_t* out_commitments48, uint64_t* out_singular,
                                  uint64_t* out_first_singular, uint64_t* out_mismatch, uint64_t* out_first_mismatch,
                                  uint64_t* out_unknown, uint64_t* out_first_unknown, uint64_t* out_segments,
                                  uint64_t* out_handle);

/* ---- device-resident inputs (what a serving loop and bench.py use: inputs already in HBM when timing starts).
 *      slot in [0, 4).  to_mont=1 stores Montgomery form (rows for commit/open), 0 canonical (MSM scalars). */
int kzg_upload_fr(kzg_ctx* ctx, int slot, const uint8_t* be32, uint64_t n, int to_mont);
int kzg_msm_resident(kzg_ctx* ctx, int slot, uint64_t n, uint64_t srs_offset, uint8_t out48[48]);
int kzg_msm_partial_resident(kzg_ctx* ctx, int slot, uint64_t n, uint64_t srs_offset, uint8_t out_xyzz192[192]);
/* Ticketed form of the two calls above: several requests in flight from ONE host thread.  submit queues the MSM on a
 * free lane and returns; wait blocks for that ticket and writes 48 (partial=0) or 192 bytes (exactly one waiter per
 * ticket).  MSM i+1's sort/accumulate then overlaps the latency-bound tail of MSM i.  Results are identical to the
 * blocking calls.  With every lane taken submit fails with KZG_E_BUSY; a blocking call made while tickets are
 * outstanding uses a free lane, or fails with KZG_E_BUSY when every lane is parked under a ticket; operations that
 * need the whole context (SRS load, kzg_upload_fr, kzg_ntt_resident) fail with KZG_E_BUSY while any ticket is out. */
int kzg_msm_submit(kzg_ctx* ctx, int slot, uint64_t n, uint64_t srs_offset, int partial, int* out_ticket);
int kzg_msm_wait(kzg_ctx* ctx, int ticket, uint8_t* out);
/* Gives up a ticket of kzg_msm_submit / kzg_msm_sharded_begin whose result will not be collected (the collective
 * between _begin and _finish raised, a peer died): drains the lane and frees it.  Without it the lane would stay parked. */
int kzg_msm_cancel(kzg_ctx* ctx, int ticket);
int kzg_commit_open_resident(kzg_ctx* ctx, uint32_t i, int slot, uint64_t T, int evaluation_form,
                             const uint8_t alpha_be32[32], uint8_t out_commitment48[48], uint8_t out_eval32[32],
                             uint8_t out_proof48[48]);
int kzg_ntt_resident(kzg_ctx* ctx, int slot, uint64_t n, int inverse); /* in place on the slot */

/* ---- pinned host staging.  acquire hands out one of four page-locked buffers of at least `bytes` bytes (it waits
 *      when all are held); release returns it.  A host that decodes the synapse's base64 text itself
 *      (zkp_subnet_amd/csrc/wire_py.c) writes the 32-byte scalars straight into it and passes the pointer as
 *      row_be32 / scalars_be32: the upload then runs at PCIe speed with no pageable bounce and no page faults, and
 *      concurrent requests each decode into their own buffer. */
int kzg_staging_acquire(kzg_ctx* ctx, uint64_t bytes, void** out_ptr, int* out_token);
int kzg_staging_release(kzg_ctx* ctx, int token);
/* Long rows: start the upload of bytes [offset, offset + bytes) of a held staging buffer NOW and return at once, so that
 * the copy engine moves tile k while the host decodes tile k + 1 of the synapse's text (the reference ships the whole
 * polynomial as text per call, neurons/miner.py:39,48).  Flushes are contiguous from offset 0 (multiples of 32 bytes).  A
 * compute call that is then handed the buffer's pointer finds the flushed prefix on the device and skips its own upload
 * (it waits for the copy on its stream, not on the host); whatever was not flushed is uploaded the ordinary way.
 * The flushes are ONE-SHOT: they serve the first compute call that is handed the pointer; a second call on the same held
 * buffer (whose bytes the holder may have rewritten) uploads the ordinary way, and the next flush starts again at
 * offset 0.  kzg_staging_release forgets the flushes. */
int kzg_staging_flush(kzg_ctx* ctx, int token, uint64_t offset, uint64_t bytes);

/* ---- where the result point is encoded.  1 (default): the XYZZ working form of the ONE point a request produces
 *      comes back in the request's single device-to-host copy and the host does the affine conversion (one Fp
 *      inversion) + ZCash compression -- a few microseconds instead of a ~140 us single-lane GPU kernel.
 *      0: encode on the GPU (k_g1_compress).  Results are identical; the *_dev entry points always stay on the GPU. */
int kzg_set_host_finish(kzg_ctx* ctx, int enable);

/* ---- per-stage HIP-event timings of the last hot-path call (events recorded on the ctx's own stream) */
enum {
    KZG_T_DECODE = 0, KZG_T_NTT, KZG_T_DIGITS, KZG_T_SCAN, KZG_T_SCATTER, KZG_T_ACCUMULATE, KZG_T_FIXUP,
    KZG_T_TREE, KZG_T_FINAL, KZG_T_POLY, KZG_T_TOTAL, KZG_T_COLLECTIVE /* kzg_msm_sharded: pack + all_gather + sum */,
    KZG_T_COUNT
};
/* enable: 0 off; 1 events around every stage (concurrent calls then serialise on one lane so that stage times stay
   attributable); 2 events around the accumulate kernel only (two per launch; nothing is serialised) */
int kzg_set_profiling(kzg_ctx* ctx, int enable);
int kzg_get_timings(kzg_ctx* ctx, float* out_ms, int count); /* accumulated over the last call's MSMs */
/* fixed-size MSM plan facts for roofline bookkeeping: entries per lane, lanes, buckets, windows */
int kzg_msm_plan(kzg_ctx* ctx, uint64_t n, int32_t out[4]);
/* The bound of the dominant kernel as a measurement of THIS device at THIS moment (SURVEY 8d "confirm on the box"):
 * k_msm_accumulate is bound by the issue rate of v_mad_u64_u32, and boxes of one pool differ by up to
 * 14 % in it.  Runs a chain of that one instruction with `waves_per_simd` waves on every SIMD for ~1.5 ms (exclusive:
 * waits for the lanes to be idle; KZG_E_BUSY while tickets are out).  out[0] ns per wave-instruction per SIMD, out[1]
 * G wave-instructions/s of the whole chip, out[2] s_memtime ticks per ns over the launch (the clock the SIMDs ran at, in
 * GHz, when s_memtime counts shader clocks), out[3] kernel ms, out[4] SIMDs, out[5] ticks per instruction of one wave.
 * bench.py calls it right after its timed region; nothing on the serving path does. */
int kzg_calibrate(kzg_ctx* ctx, int waves_per_simd, double out[6]);

/* ---- host-side wire codec (Prove.poly is a list of 43-char unpadded base64 strings, reference
 *      base/protocol.py:35-40).  packed: n x 43 chars, no separators.  Pure host code. */
int kzg_b64_decode_fr(const char* packed43, uint64_t n, uint8_t* out_be32);
int kzg_b64_encode_fr(const uint8_t* be32, uint64_t n, char* out_packed43);

#ifdef __cplusplus
}
#endif
#endif /* KZG_MI355X_H */
