// ctx.hip.h -- INTERNAL to libkzg_mi355x.so (never installed, never included by a caller): the context, its lanes and
// the helpers the translation units of the C-ABI share.  The boundary itself is include/kzg_mi355x.h; the seam it fills
// is the prover client of the reference miner (reference base/miner.py:73-84 lifecycle; neurons/miner.py:38-61 commit / open).
//
//   lanes.hip     context lifecycle, lane / ticket bookkeeping glue, record publish + host wait, staging, profiling
//   srs.hip       setup loaders (memory, file, per-device slices), synthetic SRS, window tables, read-back
//   pipeline.hip  the host-side sequencing of the kernels: one MSM (msm_core), a row's commit / open (commit_open_dev)
//   serve.hip     the serving entry points: commit / open / msm / ntt / eval, resident slots, tickets, sums
//   fr_derive.hip the kernels of kzg_rows_commit_derived: inverse-or-zero around the batched inversion, limb decomposition
//   fr_int.hip    the kernel of kzg_rows_commit_int: machine-word arithmetic on the canonical integers of resident columns
//   fr_alu.hip    the kernel of kzg_rows_commit_alu: the same arithmetic and its signed kinds, the kind chosen per cell by an op-code column
//   fr_wide.hip   the kernel of kzg_rows_commit_wide: multi-limb add, sub, mul, divmod, mulmod and the carries of its limb identity
//   fr_poseidon.hip the kernel of kzg_rows_commit_poseidon: the Hades permutation with x^5 per row, as a check, or as a round trace
//   fr_poseidon2.hip the kernel of kzg_rows_commit_poseidon2: the Poseidon2 permutation with x^5 (product-free external layer) per row, as a check, or as a round trace
//   fr_poseidon_chain.hip the kernel of kzg_rows_commit_poseidon_chain: sponge and Merkle-path chains over blocks, one lane walking each segment
//   fr_sha256.hip the kernel of kzg_rows_commit_sha256: the SHA-256 compression per row, as a check, or as a chained round trace
//   fr_keccak.hip the kernel of kzg_rows_commit_keccak: Keccak-f[1600] per row, as a check, or as a chained round trace of 64-bit lanes
//   fr_ec.hip     the kernel of kzg_rows_commit_ec: a b^-1 mod an odd p, affine point addition and doubling, the accumulator trace of a chain
//   fr_edwards.hip the kernels of kzg_rows_commit_edwards: twisted-Edwards addition over Fr itself as numerators and a denominator, the projective chain
//   fr_expr.hip   the kernel of kzg_rows_commit_expr: sums of products of rotated resident columns on H, counted and stored
//   fr_recur.hip  the scan of kzg_rows_commit_recurrence: v[t + 1] = A[t] v[t] + B[t] as a ladder over affine maps
//   fr_join.hip   the hash join of kzg_rows_commit_multiplicities, and the fetch of kzg_rows_commit_fetch that walks it
//   fr_sigma.hip  the link of kzg_rows_commit_sigma over the sorted labels, and the check of kzg_rows_check_copies
//   comm.hip      the library's own RCCL collective (kzg_comm_*, kzg_msm_sharded, the stream-chained pair)
//   abi_test.hip  unit-op test hooks (include/kzg_mi355x_test.h)
// No CPU arithmetic fallback exists anywhere here: if HIP fails, the call fails.
#pragma once
#include <hip/hip_runtime.h>

#include <errno.h>
#include <stdlib.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <new>
#include <string>
#include <system_error>
#include <thread>
#include <utility>
#include <vector>

#include "../../include/kzg_mi355x.h"
#include "../../include/kzg_mi355x_test.h"
#include "fr_kernels.hip.h"
#include "msm.hip.h"
#include "fp_lp.hip.h"
#include "rccl_dl.h"
#include "lanebook.h"
#include "rows_impl.h"

#define KZG_VERSION "kzg_mi355x 0.6 (gfx950)"
#define N_SLOTS 4
#ifndef N_LANES
#define N_LANES 4
#endif
#define N_STAGE 4
#define KZG_MAX_GATHER 4096   // partials one kzg_msm_sharded_finish can sum (ranks of a job)

void launch_calibrate_mad(hipStream_t s, uint64_t* out, uint32_t blocks, uint32_t iters);   // csrc/calibrate.hip
int calibrate_unroll();
// two spinning single-wave kernels on two streams: do they overlap?  (csrc/calibrate.hip; kzg_runtime_info)
void launch_spin_probe(hipStream_t s, uint64_t* out2, uint64_t ticks);
namespace kzg_host {  // finish_host.cpp
void xyzz_to_c48(const uint32_t* xyzz, uint8_t out48[48]);
void xyzz_pair_to_c48(const uint32_t* xyzz0, const uint32_t* xyzz1, uint8_t out0[48], uint8_t out1[48]);
void xyzz_to_partial192(const uint32_t* xyzz, uint8_t out192[192]);
// n points (56 words each, consecutive), one shared inversion
void xyzz_batch_to_c48(const uint32_t* xyzz, uint32_t n, uint8_t* out48);
}  // namespace kzg_host

namespace kzg_impl {

// device allocation that frees itself: an early error return can no longer leak it (move-only)
struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept {
        if (this != &o) {
            release();
            p = o.p; cap = o.cap;
            o.p = nullptr; o.cap = 0;
        }
        return *this;
    }
    ~DevBuf() { release(); }
    hipError_t ensure(size_t bytes) {
        if (bytes <= cap) return hipSuccess;
        release();
        size_t want = bytes + (bytes >> 3) + 256;
        hipError_t e = hipMalloc(&p, want);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            e = hipMalloc(&p, bytes);
            want = bytes;
        }
        if (e == hipSuccess) cap = want;
        else p = nullptr;
        return e;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
    template <class T>
    T* as() const { return reinterpret_cast<T*>(p); }
};

struct StageSpan {
    int stage;
    hipEvent_t a, b;
};

// A lane = everything ONE request needs: its own HIP stream, MSM workspace (sort / bucket / carry buffers), request
// buffers (uploaded row, coefficients, quotient, scan scratch) and a 1-KB "tail" record whose first half comes back to
// the host in a single copy.  A call owns its lane from acquire to release, so host threads calling into one ctx (the
// reference's axon runs Miner.forward on worker threads, neurons/miner.py:106-135) run concurrently on different lanes:
// one request's sort and latency-bound tail hide under another's accumulate.  The SRS tables are shared, read-only.
using kzg_book::LANE_CALL;      // lane / ticket / staging / row-cache bookkeeping: csrc/lanebook.h (HIP-free, TSan-driven)
using kzg_book::LANE_TICKET;
// tail record (device, 1024 B).  [0, TB_COPY) is copied to the lane's pinned buffer when a request finishes.
enum {
    TB_RES0 = 0, TB_RES1 = 224,   // result points, XYZZ working form (2 x 224 B)
    TB_EVAL = 448,                // y = f(alpha), 32 B big-endian
    TB_FLAGS = 480,               // u32 x 4: [0] bad scalar, [1] bad point, [2] longest carry run, [3] sort overflow
    TB_VERIFY = 496,              // u32: a row-cache hit whose uploaded bytes differ from the cached row's (kzg_*_cached)
    TB_C48 = 512, TB_P48 = 576,   // GPU-side encodings (host_finish off)
    TB_PART = 640,                // 192-byte partial (GPU-side packing)
    TB_COPY = 832,
    TB_ALPHA_M = 832, TB_Y_M = 864, TB_ALPHA_BE = 896, TB_SIZE = 1024
};
// the multi-row record (every call that ends in multi_msms_finish: the batched and multi-point openings, the row sets; device
// Lane::brec, pinned Lane::bpin): k + m result points in the XYZZ working form (C_0 .. C_{k-1}, pi_0 .. pi_{m-1}), the
// evaluations of up to 64 (row, point) pairs big-endian, the GPU-side encodings (host_finish off) -- [0, MR_COPY) comes back
// to the host page in one copy before the lane's ordinary record -- then the pairs' Montgomery evaluations, the points'
// Montgomery forms and the combinations' h_p(alpha_p)
#define MR_SETS (KZG_MAX_BATCH_OPEN + KZG_MAX_OPEN_POINTS)
#define MR_PAIRS (KZG_MAX_BATCH_OPEN * KZG_MAX_OPEN_POINTS)
enum {
    MR_RES = 0, MR_EVAL = MR_RES + MR_SETS * 224, MR_C48 = MR_EVAL + MR_PAIRS * 32, MR_COPY = MR_C48 + MR_SETS * 48,
    MR_Y_M = MR_COPY, MR_ALPHA_M = MR_Y_M + MR_PAIRS * 32, MR_HY_M = MR_ALPHA_M + KZG_MAX_OPEN_POINTS * 32,
    MR_SH_ALPHA_M = MR_HY_M + KZG_MAX_OPEN_POINTS * 32,   // the points of kzg_rows_commit_shplonk in Montgomery form
    MR_SIZE = MR_SH_ALPHA_M + KZG_MAX_SHPLONK_POINTS * 32
};
static_assert(MR_COPY % 4 == 0 && MR_COPY <= 8192, "the multi-row record is published by words into an 8 KB page");
static_assert(MR_PAIRS <= POLY_MAX_PAIRS && KZG_MAX_OPEN_POINTS <= POLY_MAX_POINTS, "one evaluation launch holds every pair");
#define PIN_MAXLEN 1024           // offset of the fold-depth read-back inside the lane's pinned page
#define PIN_SEQ 2048              // sequence word of the last published record (polled by finish())
#define PIN_SEQ_SORT 2052         // sequence word of the last published fold-depth / overflow pair (polled by msm_core)
struct Lane {
    int index = 0;
    hipStream_t stream = nullptr;
    DevBuf rank, sorted, hist, offsets, bufA, bufB, bufC, bufD, carries, carry_key;      // MSM workspace
    DevBuf ntt_mid;               // the vector between the passes of an NTT (9 words per element)
    DevBuf gather;                // kzg_msm_sharded_finish: the gathered partials, unpacked (own buffer: the MSM may still run)
    DevBuf comm_send, comm_recv;  // kzg_msm_sharded: this rank's packed 192-byte partial / the `world` gathered ones (sized by kzg_comm_init)
    DevBuf in_be, scal, coeffA, coeffB, qbuf, hbuf, hnext, out_be;                 // request buffers
    uint8_t* tail = nullptr;      // device, TB_SIZE
    uint8_t* pin = nullptr;       // host pinned, 4096
    uint8_t* pin_dev = nullptr;   // the same page as the GPU addresses it
    uint32_t pub_seq = 0;         // sequence number of the last record publish on this lane
    uint32_t sort_seq = 0;        // ... and of the last fold-depth publish
    bool expect_short = false;    // the request in flight is a short one (set by msm_core): finish() may poll for its record
    uint32_t expect_us = 0;       // ... and roughly how long its GPU work takes (bounds the polling)
    bool flags_clean = false;     // the tail record's flag words are zero (left so by the last request's publish)
    bool sort_ws_clean = false;   // the sort's partition counts are zero (left so by every completed sort)
    int skew_hint = 0;            // > 0: the last fast sort overflowed (skewed scalars): go straight to the exact sort
    hipEvent_t ev_sorted = nullptr, ev_done = nullptr, ev_coeffs = nullptr, ev_ext = nullptr;
    const uint8_t* in_be_src = nullptr;   // where upload_fr found the request's big-endian row on the device (in_be or a staging twin)
    hipStream_t vstream = nullptr;   // row-cache hits: upload of the caller's row + its comparison with the cached one,
    hipEvent_t ev_verify = nullptr;  // beside the request's own kernels (the lane's publish waits for this event)
    DevBuf vbuf;
    bool partial = false;         // outstanding ticket wants the 192-byte partial
    // the multi-row calls: their record (MR_*; device brec + the 8 KB pinned, mapped page bpin below), the coefficients of rows
    // that arrived in evaluation form, and the openings' combinations h_p (the builders: a scratch vector) -- allocated by the
    // first such call on the lane
    DevBuf brec, bcoef, bcomb;
    // kzg_rows_commit_quotient: the rows' (and L_0's) evaluations on the coset, one vector of E T elements each, and the
    // staging vector the extensions and the pointwise result pass through -- allocated by the first quotient call on the lane
    DevBuf qext, qstage;
    uint8_t* bpin = nullptr;
    uint8_t* bpin_dev = nullptr;
    // profiling spans of the call running on this lane
    std::vector<hipEvent_t> ev_pool;
    size_t ev_used = 0;
    std::vector<StageSpan> spans;
    g1_xyzz_t* res() const { return reinterpret_cast<g1_xyzz_t*>(tail + TB_RES0); }
    uint32_t* flags() const { return reinterpret_cast<uint32_t*>(tail + TB_FLAGS); }
};
struct Stage {
    void* p = nullptr;
    size_t cap = 0;               // (who holds the buffer is the book's business: ctx->book.stage_*)
    // kzg_staging_flush: a device twin that receives the buffer's prefix WHILE the host is still decoding the rest
    DevBuf twin;
    uint64_t flushed = 0;         // bytes [0, flushed) of p are in (or on their way to) the twin
    uint64_t consumed_by = 0;     // id of the API call that was served from the twin (0: none yet).  The flushes are ONE-SHOT:
                                  // a later call handed the same pointer (the holder may have rewritten the buffer) uploads
                                  // the ordinary way, and the next flush starts again from offset 0
    hipEvent_t ev = nullptr;      // recorded on ctx->h2d behind the last flush
    // the pointer as OTHER threads may read it (flushed_twin scans every record; only the holder touches the rest)
    std::atomic<void*> p_pub{nullptr};
};

}  // namespace kzg_impl

struct kzg_ctx {
    int device = 0;
    kzg_book::LaneBook<N_LANES, N_STAGE> book;   // lanes, tickets, staging pool, row-cache slots: csrc/lanebook.h
    std::mutex mu;                 // guards the twiddle caches, config and timings
    int c_user = 0, c = 0, nwin = 0;
    int poll_timeout_ms = 200;   // finish(): how long the pinned page is polled before falling back to the stream
    WinLayout lay;
    uint32_t nbuckets = 0;
    // resident SRS + window tables: table[w*stride + j] = 2^off[w] P_j   (read-only while any lane is busy)
    kzg_impl::DevBuf table;
    uint64_t stride = 0, T = 0;
    int scale = 0, mscale = 0;
    kzg_impl::Lane lane[N_LANES];
    kzg_impl::DevBuf slot[N_SLOTS];
    uint64_t slot_n[N_SLOTS] = {0, 0, 0, 0};
    int slot_mont[N_SLOTS] = {0, 0, 0, 0};
    std::map<int, kzg_impl::DevBuf> tw_fwd, tw_inv, inv_n;
    std::map<int, kzg_impl::DevBuf> quot_consts;   // kzg_rows_commit_quotient's constants, by log T * 4 + ext_log (under mu)
    kzg_impl::Stage stage[N_STAGE];
    hipStream_t h2d = nullptr;     // the copy stream of kzg_staging_flush (one for all staging buffers: they share the link)
    // kzg_g1_sum*: own stream and buffers, independent of the lanes
    std::mutex aux_mu;
    hipStream_t aux = nullptr;
    kzg_impl::DevBuf aux_in, aux_pts, aux_out;
    uint8_t* aux_pin = nullptr;
    // the library's own communicator (kzg_comm_*): one ncclAllGather of 192 B per rank per sharded MSM, on the lane's stream
    struct Comm {
        std::mutex mu;            // RCCL allows one thread at a time per communicator: guards every call that names `comm`
        ncclComm_t comm = nullptr;
        hipStream_t first_stream = nullptr;   // the stream kzg_comm_init's first (connecting) all_gather ran on; lives with `comm`
        int rank = 0, world = 0;
        int timeout_ms = 0;       // kzg_comm_set_timeout (0: wait for ever)
        bool broken = false;      // a collective failed or timed out and the communicator was aborted
        uint64_t gen = 0;         // bumped whenever `comm` is installed, aborted or dropped: a sharded MSM compares the value it
                                  // started under with the one it finds after its wait (another lane's timeout may have aborted
                                  // the communicator UNDER its collective: the stream then ran on over stale bytes)
        std::string why;
        std::atomic<int> stall_ms{0};   // kzg_test_comm_stall: the next `stall_left` sharded MSMs spin this long first
        std::atomic<int> stall_left{0};
    } comm;
    int profiling = 0;   // 0 off, 1 every stage (calls serialise on lane 0), 2 the accumulate kernel only (no serialisation)
    bool host_finish = true;
    bool srs_subgroup_check = true;  // kzg_load_srs*: G1 membership of every point (kzg_set_srs_subgroup_check)
    float tms[KZG_T_COUNT] = {0};  // stage times of the last completed hot-path call
    double load_stats[4] = {0, 0, 0, 0};   // kzg_get_load_stats
    int32_t rt_info[4] = {0, 0, 0, 0};     // kzg_runtime_info: measured once by kzg_create
    // coefficient vectors of the last few rows, keyed by the caller's 128-bit content tag (kzg_commit_cached /
    // kzg_open_cached): the reference miner sends the SAME row twice per request (neurons/miner.py:56-61)
    // (which slot holds which row, and who is using it: ctx->book.rcache_*)
    struct RowCache {
        kzg_impl::DevBuf coef;
        kzg_impl::DevBuf raw;        // the row's 32-byte big-endian elements as they were uploaded: what a hit is verified against
    } rcache[N_LANES];
    // committed row sets (kzg_rows_commit / kzg_rows_open / kzg_rows_release; serve.hip).  A set keeps the coefficients of
    // its k rows in its own buffer.  `refs` counts the running opens that read it: a release under an open only unlinks the
    // handle, and the buffer goes to `sets_free` when the last such open ends.  Released buffers are kept and reused by
    // capacity (no hipFree on the request path while other lanes run); the free list is trimmed by an SRS (re)load, which
    // holds every lane and also frees the buffers of the sets it makes stale.
    struct RowSet {
        uint32_t i = 0, k = 0;
        uint64_t T = 0;
        kzg_impl::DevBuf buf;        // k x T Montgomery coefficients, row-major (empty once stale)
        int refs = 0;
        bool stale = false;          // committed under an SRS that has since been replaced
        bool released = false;       // handle unlinked; the buffer waits for refs == 0
        // a quotient accumulator (kzg_rows_quotient_part): an entry of this table like a set -- handle, cap, stats, staleness,
        // release, free list -- that is NOT a row set: buf holds the N = T << acc_ext_log canonical values of sum_p scale_p
        // num_p / Z_H on the coset, k is 0, and every call that takes row sets refuses it.  acc_mu serialises the adds of parts
        // that run on several lanes (taken behind the lane, in front of sets_mu; held from an add's launch to its completion).
        bool acc = false;
        uint32_t acc_ext_log = 0;
        std::unique_ptr<std::mutex> acc_mu;
    };
    std::mutex sets_mu;              // guards everything below
    std::map<uint64_t, RowSet> sets; // by handle: live sets, and released ones that an open still reads
    uint32_t sets_pending = 0;       // commits between their reservation and their insertion (count against the cap)
    std::vector<kzg_impl::DevBuf> sets_free;
};

namespace kzg_impl {

// ---- errors: the message of the last failing call ON THIS THREAD (calls run concurrently: a per-ctx string would be torn)
int fail(kzg_ctx* ctx, int code, const std::string& msg);
const char* last_error_cstr();
#define HIPCHK(ctx, expr)                                                                                   \
    do {                                                                                                    \
        hipError_t _e = (expr);                                                                             \
        if (_e != hipSuccess)                                                                               \
            return fail(ctx, _e == hipErrorOutOfMemory ? KZG_E_NOMEM : KZG_E_HIP,                           \
                        std::string(#expr) + ": " + hipGetErrorString(_e));                                 \
    } while (0)
// the API call running on this thread: a fresh id whenever a call takes its lane(s) (LaneHold::take*).  What a one-shot
// resource (the flushed twin of a staging buffer) remembers of the call it served.
uint64_t call_id_new();
uint64_t call_id_current();

// ---- lane ownership (lanes.hip; the state machine itself is csrc/lanebook.h)
int lane_acquire(kzg_ctx* ctx, int state, int* out_li);
int lane_try_second(kzg_ctx* ctx, int first);
void lane_release(kzg_ctx* ctx, int li);
int lanes_acquire_all(kzg_ctx* ctx);
void lanes_release_all(kzg_ctx* ctx);
int ticket_claim(kzg_ctx* ctx, int ticket);
// Owns one lane (optionally a second) for the duration of a call.  Unless the call reached its normal end (`clean`),
// the streams are drained before the lanes become reusable: a HIP failure midway leaves kernels queued that still read
// and write the lane's buffers.
struct LaneHold {
    kzg_ctx* ctx;
    int li = -1, li2 = -1;
    bool all = false, clean = false;
    explicit LaneHold(kzg_ctx* c) : ctx(c) {}
    LaneHold(const LaneHold&) = delete;
    LaneHold& operator=(const LaneHold&) = delete;
    int take() {
        (void)call_id_new();
        return lane_acquire(ctx, LANE_CALL, &li);
    }
    int take_all() {
        (void)call_id_new();
        int rc = lanes_acquire_all(ctx);
        if (rc == KZG_OK) { all = true; li = 0; }
        return rc;
    }
    Lane& L() { return ctx->lane[li]; }
    Lane* second() {
        if (li2 < 0) li2 = lane_try_second(ctx, li);
        return li2 >= 0 ? &ctx->lane[li2] : nullptr;
    }
    void drain();     // wait for everything this call queued (what the destructor does for a call that did not end cleanly)
    ~LaneHold();
};

// ---- per-stage HIP-event spans (kzg_set_profiling)
hipEvent_t prof_event(Lane& L);
struct Span {
    Lane* lane = nullptr;
    int idx = -1;
    hipStream_t stream;
    Span(kzg_ctx* c, Lane& L, int stage, hipStream_t st = nullptr) : stream(st ? st : L.stream) {
        if (!c->profiling || (c->profiling == 2 && stage != KZG_T_ACCUMULATE)) return;
        lane = &L;
        StageSpan s{stage, prof_event(L), prof_event(L)};
        (void)hipEventRecord(s.a, stream);
        L.spans.push_back(s);
        idx = (int)L.spans.size() - 1;
    }
    ~Span() {
        if (idx >= 0) (void)hipEventRecord(lane->spans[idx].b, stream);
    }
};
void prof_begin(kzg_ctx* ctx, Lane& L);   // opens the KZG_T_TOTAL span of the call on lane L
void prof_close(kzg_ctx* ctx, Lane& L);   // ... ends it just before the last copy-back
void prof_end(kzg_ctx* ctx, Lane& L);     // lane stream already synchronised: stage times -> ctx->tms

// ---- ending a request (lanes.hip)
// waits until the pinned word at `off` shows `seq` (a k_publish has landed); false if it does not within the budget
bool poll_pinned(const kzg_ctx* ctx, const Lane& L, uint32_t off, uint32_t seq);
int need_srs(kzg_ctx* ctx);
int clear_flags(kzg_ctx* ctx, Lane& L);
int finish(kzg_ctx* ctx, Lane& L, bool allow_poll = true);
void result_c48(kzg_ctx* ctx, Lane& L, int which, uint8_t out48[48]);
void result_partial(kzg_ctx* ctx, Lane& L, uint8_t out192[192]);
void queue_encode(kzg_ctx* ctx, Lane& L, bool first, bool second);
void queue_pack(kzg_ctx* ctx, Lane& L);

// ---- the kernel sequences (pipeline.hip)
inline int ilog2_exact(uint64_t n) {
    if (!n || (n & (n - 1))) return -1;
    int l = 0;
    while (((uint64_t)1 << l) < n) l++;
    return l;
}
int pick_chunk(uint64_t entries);
// sc's MSMs over points [srs_offset, srs_offset + n) as one pass on lane L -> out_xyzz[0 .. sc.nsets()); KZG_E_ARG, with
// nothing queued, for a malformed sc: no sets, a count without scalars, more sets than min(MSM_MAX_SETS, msm_sort_max_sets(c))
int msm_core(kzg_ctx* ctx, Lane& L, const ScalarSets& sc, uint64_t n, uint64_t srs_offset, g1_xyzz_t* out_xyzz);
// how a multi-row call's k row sets + m tail sets (its quotients) go through msm_core: pass p takes rows [row0, row0 + nrows)
// and tail sets [tail0, tail0 + ntail), on the call's lane (lane 0) or its second one.  Pure: window c, nbuckets per set,
// long_rows = past KZG_BATCHED_ROW_MAX.  out: room for k + m passes; returns their number.
struct MsmPass {
    uint32_t row0, nrows, tail0, ntail, lane;
};
uint32_t plan_msm_passes(int c, uint32_t nbuckets, bool long_rows, uint32_t k, uint32_t m, MsmPass* out);
int ensure_twiddles(kzg_ctx* ctx, Lane& L, int log_n, int inverse, uint32_t** tw, uint32_t** invn);
int row_to_coeffs(kzg_ctx* ctx, Lane& L, const uint32_t* row_dev, uint64_t T, int evaluation_form, const uint32_t** coeffs,
                  uint32_t* dst = nullptr);
int check_worker(kzg_ctx* ctx, uint32_t i, uint64_t T);
const uint8_t* flushed_twin(kzg_ctx* ctx, const uint8_t* host_ptr, uint64_t bytes, hipEvent_t* ev);
int upload_fr(kzg_ctx* ctx, Lane& L, const uint8_t* be32, uint64_t n, uint32_t* dst, int to_mont);
struct VerifyJob {   // a row-cache hit's evidence: the caller's row (host) against the bytes the slot was filled from (device)
    const uint8_t* row_be32;
    uint64_t T;
    const uint32_t* cached_raw;
};
int commit_open_dev(kzg_ctx* ctx, LaneHold& H, uint32_t i, const uint32_t* row_dev, uint64_t T, int evaluation_form,
                    const uint8_t* alpha_be32, uint8_t* out_c48, uint8_t* out_eval32, uint8_t* out_p48,
                    const uint32_t* coeffs_ready = nullptr, uint32_t* coeffs_dst = nullptr, const VerifyJob* verify = nullptr);
// k rows (Montgomery, k x T elements at row_dev) of worker i, one point alpha, one challenge gamma: the k commitments, the k
// evaluations and ONE proof for h = sum_j gamma^j f_j (kzg_commit_open_batch)
int commit_open_batch_dev(kzg_ctx* ctx, LaneHold& H, uint32_t i, const uint32_t* rows_dev, uint32_t k, uint64_t T,
                          int evaluation_form, const uint8_t* alpha_be32, const uint8_t* gamma_be32, uint8_t* out_c48,
                          uint8_t* out_evals32, uint8_t* out_p48);
// k rows of worker i opened at m points (kzg_commit_open_multi): masks[p] names point p's rows, gammas their challenge;
// the k commitments, the evaluations of every masked pair (point-major) and one proof per point
int commit_open_multi_dev(kzg_ctx* ctx, LaneHold& H, uint32_t i, const uint32_t* rows_dev, uint32_t k, uint64_t T,
                          int evaluation_form, uint32_t m, const uint8_t* points_be32, const uint32_t* masks,
                          const uint8_t* gammas_be32, uint8_t* out_c48, uint8_t* out_evals32, uint8_t* out_p48);

// committed row sets: the commit's INTT into the set's buffer dst and its k MSMs; the open of rows read through rt
int rows_commit_dev(kzg_ctx* ctx, LaneHold& H, uint32_t i, const uint32_t* rows_dev, uint32_t k, uint64_t T,
                    int evaluation_form, uint32_t* dst, uint8_t* out_c48);
int rows_open_dev(kzg_ctx* ctx, LaneHold& H, uint32_t i, const RowTab& rt, uint32_t k, uint64_t T, uint32_t m,
                  const uint8_t* points_be32, const uint32_t* masks, const uint8_t* gammas_be32, uint8_t* out_evals32,
                  uint8_t* out_p48);
// the evaluations of the masked pairs only (kzg_rows_eval); the caller-weighted openings (kzg_rows_open_lincomb: masks[p] =
// the rows with a nonzero coefficient at point p, coeffs_be32 m x k point-major)
int rows_eval_dev(kzg_ctx* ctx, LaneHold& H, uint32_t i, const RowTab& rt, uint32_t k, uint64_t T, uint32_t m,
                  const uint8_t* points_be32, const uint32_t* masks, uint8_t* out_evals32);
int rows_lincomb_dev(kzg_ctx* ctx, LaneHold& H, uint32_t i, const RowTab& rt, uint32_t k, uint64_t T, uint32_t m,
                     const uint8_t* points_be32, const uint8_t* coeffs_be32, const uint32_t* masks, uint8_t* out_values32,
                     uint8_t* out_p48);
// kzg_rows_commit_shplonk: the rows with one point set S form a group (rows: their mask; pt: S, ascending); the caller hands
// the groups over sorted by descending npts, so that the groups still dividing in pass d are a prefix of every batch.
// h = sum_groups quot(sum_{j in group} c_j f_j, Z_S) goes into the new one-row set's buffer dst; its commitment to out_c48.
struct ShGroup {
    uint32_t rows;
    uint8_t npts, pt[KZG_MAX_SHPLONK_POINTS];
};
int rows_shplonk_dev(kzg_ctx* ctx, LaneHold& H, uint32_t i, const RowTab& rt, uint32_t k, uint64_t T, uint32_t m,
                     const uint8_t* points_be32, const uint8_t* coeffs_be32, uint32_t n_groups, const ShGroup* groups,
                     uint32_t* dst, uint8_t* out_c48);
// The selectors of a kzg_rows_commit_*_sel builder (checked by the caller): the n DISTINCT resident rows the call names
// (coefficients, like every row of a set) and, per lookup, which of them is its q_l (SEL_NONE: the constant 1, the lookup runs
// through the kernels of the call without selectors).  Null, or every entry SEL_NONE: the builder without selectors.
#define SEL_NONE 0xffu
struct SelPlan {
    uint32_t n;
    const uint32_t* row[POLY_MAX_ROWS];
    uint8_t of[POLY_MAX_ROWS];
};
// the grand product of k wire / sigma row pairs (rows read through the two tables) into a new one-row set's buffer dst:
// its commitment, the closing value, and whether some denominator was zero (z undefined: the caller creates no set)
int rows_grand_product_dev(kzg_ctx* ctx, LaneHold& H, uint32_t i, const RowTab& wires, const RowTab& sigmas, uint32_t k,
                           uint64_t T, const uint8_t* shifts_be32, const uint8_t* beta_be32, const uint8_t* gamma_be32,
                           uint32_t* dst, uint8_t* out_c48, uint8_t* out_closing32, bool* out_zero_den,
                           const Blind* zk = nullptr, const uint8_t* start_be32 = nullptr);
// The selectors of kzg_rows_commit_shuffle (checked by the caller): per group the resident row (coefficients) that is q_g on
// the input side and q'_g on the shuffle side; null: the side has no selector there
struct ShuffleSel {
    const uint32_t *in[POLY_MAX_ROWS], *sh[POLY_MAX_ROWS];
};
// the shuffle grand product of n_groups x width input rows against as many shuffle rows into a new one-row set's buffer dst:
// its commitment, the closing value, and whether some denominator was zero (z undefined: the caller creates no set)
int rows_shuffle_dev(kzg_ctx* ctx, LaneHold& H, uint32_t i, const RowTab& inputs, const RowTab& shuffles, uint32_t n_groups,
                     uint32_t width, uint64_t T, const uint8_t* theta_be32, const uint8_t* gamma_be32, uint32_t* dst,
                     uint8_t* out_c48, uint8_t* out_closing32, bool* out_zero_den, const Blind* zk, const ShuffleSel* sel);
// the lookup running sum over n_lookups x width input rows, width table rows and the multiplicity row `mult` into a new one-row
// set's buffer dst: its commitment, the closing value, and whether some denominator was zero (the caller creates no set)
int rows_lookup_sum_dev(kzg_ctx* ctx, LaneHold& H, uint32_t i, const RowTab& inputs, const RowTab& table, const uint32_t* mult,
                        uint32_t n_lookups, uint32_t width, uint64_t T, const uint8_t* theta_be32, const uint8_t* beta_be32,
                        uint32_t* dst, uint8_t* out_c48, uint8_t* out_closing32, bool* out_zero_den, const Blind* zk = nullptr,
                        const SelPlan* sel = nullptr);
// the lookup multiplicities of n_lookups x width input rows against width table rows into a new one-row set's buffer dst: its
// commitment, the number of cells whose tuple is no table row, and whether a probe walk reached its bound (no set then)
int rows_multiplicities_dev(kzg_ctx* ctx, LaneHold& H, uint32_t i, const RowTab& inputs, const RowTab& table, uint32_t n_lookups,
                            uint32_t width, uint64_t T, uint32_t* dst, uint8_t* out_c48, uint64_t* out_missing,
                            bool* out_overrun, const Blind* zk = nullptr, const SelPlan* sel = nullptr);
// the `width` input rows, stably sorted as tuples by their first n_keys columns, into a new width-row set's buffer dst: their
// commitments.  lay (null: all T rows are sorted): rows [0, usable) are sorted, rows usable + s of column c take
// tail_be32[c * (T - usable) + s] (checked by the caller: 1 <= usable < T, T - usable <= KZG_MAX_BLIND_ROWS, canonical scalars)
int rows_sorted_dev(kzg_ctx* ctx, LaneHold& H, uint32_t i, const RowTab& inputs, uint32_t width, uint32_t n_keys, uint64_t T,
                    uint32_t* dst, uint8_t* out_c48, const Blind* lay);
// the n_out helper rows of the n_ops ops (checked by the caller: kinds, rows inside `inputs`, bits and counts in range, the
// counts summing to n_out) into a new n_out-row set's buffer dst: their commitments and one count per op (zero cells of an
// inv0 op, cells at or above 2^(bits count) of a limbs op).  lay: as for rows_sorted_dev, the tail column-major over n_out
int rows_derived_dev(kzg_ctx* ctx, LaneHold& H, uint32_t i, const RowTab& inputs, uint32_t n_ops, const kzg_derive_op* ops,
                     uint32_t n_out, uint64_t T, uint32_t* dst, uint8_t* out_c48, uint64_t* out_counts, const Blind* lay);
// the n_out rows of the n_ops integer ops (checked by the caller: kinds, widths, counts summing to n_out, rows inside `inputs`,
// immediates that fit) into a new n_out-row set's buffer dst: their commitments and, per op, the number of cells read with an
// operand out of range and the smallest such row (KZG_INT_NONE: none).  lay: as for rows_derived_dev
int rows_int_dev(kzg_ctx* ctx, LaneHold& H, uint32_t i, const RowTab& inputs, uint32_t n_ops, const kzg_int_op* ops, uint32_t n_out,
                 uint64_t T, uint32_t* dst, uint8_t* out_c48, uint64_t* out_counts, uint64_t* out_first, const Blind* lay);
// the n_out rows of the n_units units over one program of n_entries entries (checked by the caller: kinds, widths, immediates,
// counts summing to n_out, rows inside `inputs`) into a new n_out-row set's buffer dst: their commitments and, per unit, four
// words in out_stats: [u] the cells with an operand out of range, [n_units + u] the cells with an unknown op-code, [2 n_units
// + u] and [3 n_units + u] the smallest such rows (KZG_ALU_NONE: none).  lay: as for rows_derived_dev
int rows_alu_dev(kzg_ctx* ctx, LaneHold& H, uint32_t i, const RowTab& inputs, uint32_t n_entries, const kzg_alu_entry* program,
                 uint32_t n_units, const kzg_alu_unit* units, uint32_t n_out, uint64_t T, uint32_t* dst, uint8_t* out_c48,
                 uint64_t* out_stats, const Blind* lay);
// the n_out rows of the n_ops multi-limb ops (checked by the caller: kinds, b, L, counts summing to n_out, operands inside
// `inputs`, immediates that fit, m != 0) into a new n_out-row set's buffer dst: their commitments and four runs of n_ops
// statistics (out-of-range rows, quotient-over or inexact rows, and the smallest row of each, KZG_INT_NONE: none).  lay: as for
// rows_derived_dev
int rows_wide_dev(kzg_ctx* ctx, LaneHold& H, uint32_t i, const RowTab& inputs, uint32_t n_ops, const kzg_wide_op* ops,
                  uint32_t n_out, uint64_t T, uint32_t* dst, uint8_t* out_c48, uint64_t* out_stats, const Blind* lay);
// the n_out committed columns of the n_units Poseidon units (checked by the caller: t, R_F, R_P, periods, canonical constants and
// immediates, modes, flags, out lists, rows inside `inputs`) into a new n_out-row set's buffer dst (null when n_out = 0: then no
// transform back and no MSM runs): their commitments and two runs of n_units statistics (the mismatching rows of a check and the
// smallest of them, KZG_POSEIDON_NONE: none).  lay: as for rows_derived_dev
int rows_poseidon_dev(kzg_ctx* ctx, LaneHold& H, uint32_t i, const RowTab& inputs, const kzg_poseidon_params* params,
                      uint32_t n_units, const kzg_poseidon_unit* units, uint32_t n_out, uint64_t T, uint32_t* dst,
                      uint8_t* out_c48, uint64_t* out_stats, const Blind* lay);
// rows_poseidon_dev with the Poseidon2 parameters (checked by the caller: t in {2, 3, 4, 8}, R_F, R_P, periods of at least R + 2,
// canonical constants); the units, the statistics and lay are rows_poseidon_dev's
int rows_poseidon2_dev(kzg_ctx* ctx, LaneHold& H, uint32_t i, const RowTab& inputs, const kzg_poseidon2_params* params,
                       uint32_t n_units, const kzg_poseidon_unit* units, uint32_t n_out, uint64_t T, uint32_t* dst,
                       uint8_t* out_c48, uint64_t* out_stats, const Blind* lay);
// the n_out committed columns of the n_units SHA-256 units (checked by the caller: modes, flags, periods, out lists, rows inside
// `inputs`) into a new n_out-row set's buffer dst (null when n_out = 0: then no transform back and no MSM runs): their
// commitments and five runs of n_units statistics (over-range cells, mismatching rows, messages, then the smallest row of the
// first and of the second kind, KZG_SHA256_NONE: none).  lay: as for rows_derived_dev
int rows_sha256_dev(kzg_ctx* ctx, LaneHold& H, uint32_t i, const RowTab& inputs, uint32_t n_units, const kzg_sha256_unit* units,
                    uint32_t n_out, uint64_t T, uint32_t* dst, uint8_t* out_c48, uint64_t* out_stats, const Blind* lay);
// the n_out committed columns of the n_units Keccak units (checked by the caller: modes, flags, periods, rates, out lists, rows
// inside `inputs`) into a new n_out-row set's buffer dst (null when n_out = 0: then no transform back and no MSM runs): their
// commitments and five runs of n_units statistics (over-range cells, mismatching rows, messages, then the smallest row of the
// first and of the second kind, KZG_KECCAK_NONE: none).  lay: as for rows_derived_dev
int rows_keccak_dev(kzg_ctx* ctx, LaneHold& H, uint32_t i, const RowTab& inputs, uint32_t n_units, const kzg_keccak_unit* units,
                    uint32_t n_out, uint64_t T, uint32_t* dst, uint8_t* out_c48, uint64_t* out_stats, const Blind* lay);
// the n_out committed rows of the n_units elliptic-curve units over `curve` (checked by the caller: the curve, modes, flags,
// names, operand runs inside `inputs`) into a new n_out-row set's buffer dst (null when n_out = 0: then no transform back and no
// MSM runs): their commitments and seven runs of n_units statistics (out-of-range rows, exceptional rows, mismatching rows or
// on a CHAIN unit unknown op-codes, segments, then the smallest row of the first three kinds, KZG_EC_NONE: none).  lay: as for
// rows_derived_dev
int rows_ec_dev(kzg_ctx* ctx, LaneHold& H, uint32_t i, const RowTab& inputs, const kzg_ec_curve* curve, uint32_t n_units,
                const kzg_ec_unit* units, uint32_t n_out, uint64_t T, uint32_t* dst, uint8_t* out_c48, uint64_t* out_stats,
                const Blind* lay);
// the n_out committed rows of the n_units twisted-Edwards units over `curve` (checked by the caller: the curve, canonical
// immediates, modes, flags, names, out orders, rows inside `inputs`) into a new n_out-row set's buffer dst (null when n_out =
// 0: then no inversion, no transform back and no MSM runs): their commitments and five runs of n_units statistics (exceptional
// rows or steps, mismatching rows or on a CHAIN unit unknown op-codes, segments, then the smallest row of the first two kinds,
// KZG_EDWARDS_NONE: none).  lay: as for rows_derived_dev
int rows_edwards_dev(kzg_ctx* ctx, LaneHold& H, uint32_t i, const RowTab& inputs, const kzg_edwards_curve* curve,
                     uint32_t n_units, const kzg_edwards_unit* units, uint32_t n_out, uint64_t T, uint32_t* dst, uint8_t* out_c48,
                     uint64_t* out_stats, const Blind* lay);
// the n_out committed columns of the n_units Poseidon chain units (checked by the caller: params as for rows_poseidon_dev, modes,
// layouts, periods, column ids, digests, canonical immediates, rows inside `inputs`) into a new n_out-row set's buffer dst (null
// when n_out = 0: then no transform back and no MSM runs): their commitments and five runs of n_units statistics (segments, bad
// positions, mismatching segments, then the smallest row of the last two kinds, KZG_POSEIDON_NONE: none).  lay: as for
// rows_derived_dev
int rows_poseidon_chain_dev(kzg_ctx* ctx, LaneHold& H, uint32_t i, const RowTab& inputs, const kzg_poseidon_params* params,
                            uint32_t n_units, const kzg_poseidon_chain_unit* units, uint32_t n_out, uint64_t T, uint32_t* dst,
                            uint8_t* out_c48, uint64_t* out_stats, const Blind* lay);
// the n_out committed ones of the n_exprs expressions (checked by the caller: term counts and lengths in range, rows inside
// `inputs`, rotations reduced into [0, T), canonical coefficients; is_check[e] != 0: expression e is only counted) into a new
// n_out-row set's buffer dst (null when n_out = 0: then no transform back and no MSM runs): their commitments, and per
// expression the number of non-zero cells among the rows evaluated and the smallest such row (KZG_EXPR_NONE: none).  lay: as
// for rows_sorted_dev, the tail column-major over the n_out committed columns
int rows_expr_dev(kzg_ctx* ctx, LaneHold& H, uint32_t i, const RowTab& inputs, uint32_t n_exprs, const ExprPlan* exprs,
                  const uint8_t* is_check, uint32_t n_out, uint64_t T, uint32_t* dst, uint8_t* out_c48, uint64_t* out_nonzero,
                  uint64_t* out_first, const Blind* lay);
// one recurrence of kzg_rows_commit_recurrence: v[0] = start, v[t + 1] = mul[t] v[t] + add[t]; a side with n_terms = 0 is empty
// (mul: the constant 1, add: the constant 0); the rest of each side as the caller of rows_expr_dev checks an expression
struct RecurSpec {
    ExprPlan mul, add;
    const uint8_t* start_be32;   // a canonical scalar, 32 big-endian HOST bytes
};
// the n_recs recurrences into a new n_recs-row set's buffer dst: their commitments and closing values (32 big-endian bytes
// each).  lay (null: rows 0 .. T - 1 hold v[0] .. v[T - 1] and the closing value is v[T]): the _zk layout -- rows 0 .. usable
// hold v[0] .. v[usable], the last of them the closing value, and row usable + 1 + s of column c takes
// tail_be32[c * (T - usable - 1) + s] (checked by the caller as blind_check does, over n_recs columns)
int rows_recur_dev(kzg_ctx* ctx, LaneHold& H, uint32_t i, const RowTab& inputs, uint32_t n_recs, const RecurSpec* recs, uint64_t T,
                   uint32_t* dst, uint8_t* out_c48, uint8_t* out_closing32, const Blind* lay);
// the n_reads reads of kzg_rows_commit_fetch (checked by the caller: n_keys <= w_tab rows in `table`, n_reads max(n_keys, 1)
// rows in `inputs`, n_reads (w_tab - n_keys + index) in [1, KZG_MAX_BATCH_OPEN], no index with n_keys = 0, T <= 2^27) into a
// new set's buffer dst: their commitments, per read the number of cells without a table row and the smallest such cell
// (KZG_FETCH_NONE: none), and whether a walk of the join reached its bound (the caller creates no set).  lay: as for
// rows_sorted_dev, the tail column-major over all output columns; cells and table rows at or behind `usable` do not take part
int rows_fetch_dev(kzg_ctx* ctx, LaneHold& H, uint32_t i, const RowTab& inputs, const RowTab& table, uint32_t n_reads,
                   uint32_t n_keys, uint32_t w_tab, bool index, uint64_t T, uint32_t* dst, uint8_t* out_c48, uint64_t* out_missing,
                   uint64_t* out_first, bool* out_overrun, const Blind* lay);
// the sigma columns of the k label rows (checked by the caller: k in [1, KZG_MAX_BATCH_OPEN], 1 <= n <= T, k n <= 2^27, canonical
// shifts and free label; n < T: rows [n, T) map to themselves and their labels are not read) into a new k-row set's buffer dst:
// their commitments, the number of classes and the number of cells t < n that map to themselves.  free_be32 null: no free label
int rows_sigma_dev(kzg_ctx* ctx, LaneHold& H, uint32_t i, const RowTab& labels, uint32_t k, uint64_t T, uint64_t n,
                   const uint8_t* shifts_be32, const uint8_t* free_be32, uint32_t* dst, uint8_t* out_c48, uint64_t* out_stats);
// the copy constraints of the same labels checked against the k wire rows: out[0] the cells whose value differs from that of
// their class's smallest cell, out[1] the smallest such flat index c T + t (UINT64_MAX: none).  No set, no MSM
int rows_check_copies_dev(kzg_ctx* ctx, LaneHold& H, uint32_t i, const RowTab& wires, const RowTab& labels, uint32_t k, uint64_t T,
                          uint64_t n, const uint8_t* free_be32, uint64_t* out);
// the quotient pieces of the constraints qp over the n_rows coefficient rows of rt into a new n_pieces-row set's buffer dst:
// their commitments, and whether a coefficient of t at or above n_pieces T was not zero (the caller creates no set)
int rows_quotient_dev(kzg_ctx* ctx, LaneHold& H, uint32_t i, const RowTab& rt, uint32_t n_rows, uint64_t T, const QuotPlan& qp,
                      uint32_t n_pieces, uint32_t* dst, uint8_t* out_c48, bool* out_bad_shape);
// kzg_rows_quotient_part / _finish: the quotient call cut in two around an accumulator of N = T << ext_log canonical values.
// front: the part's num / Z_H into the lane's staging vector.  add: acc (+)= scale * that vector as the call's last device
// step (the caller holds the accumulator's mutex around it).  finish: the inverse transform, the pieces with the shape check
// and the MSM pass over `src`, which is only read (the accumulator, or the single call's staging vector)
int rows_quotient_front_dev(kzg_ctx* ctx, LaneHold& H, const RowTab& rt, uint32_t n_rows, uint64_t T, const QuotPlan& qp);
int rows_quotient_add_dev(kzg_ctx* ctx, LaneHold& H, uint64_t T, uint32_t ext_log, const uint8_t* scale_be32, uint32_t* acc,
                          bool first);
int rows_quotient_finish_dev(kzg_ctx* ctx, LaneHold& H, uint32_t i, uint64_t T, int ext_log, const uint32_t* acc, uint32_t n_pieces,
                             uint32_t* dst, uint8_t* out_c48, bool* out_bad_shape);
// an SRS (re)load is installing a new table (every lane held): marks every live set stale, frees its buffer and the free list
void rows_invalidate(kzg_ctx* ctx);
// (the entries behind the kzg_rows_* / kzg_multi_rows_* exports, Blind and SelCall: rows_impl.h)

// ---- the collective (comm.hip)
void comm_teardown(kzg_ctx* ctx);

}  // namespace kzg_impl
