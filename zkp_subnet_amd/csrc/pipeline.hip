// pipeline.hip -- the host-side sequencing of the HIP kernels: ONE Pippenger MSM on a lane (msm_core: sort -> accumulate ->
// fold -> tree -> final; kernels in msm_sort / msm_accumulate / msm_tree.hip) and one worker row's commit and / or open (commit_open_dev: INTT -> MSM ||
// evaluation + quotient -> MSM; kernels in fr_ntt.hip / fr_poly.hip).  What it computes is what the reference's prover computes behind
// Client.worker_commit / worker_open (reference neurons/miner.py:38-54); see ctx.hip.h for the map of the library.
#include "ctx.hip.h"

using namespace kzg_impl;

namespace kzg_impl {

// sorted entries per accumulate lane.  Large MSMs (throughput-bound): the grid is a whole number of "rounds" of 131072
// lanes (2 waves per SIMD on 256 CUs: the second wave hides the point loads) so that the last round is not a partially
// filled tail; chunks stay <= 512 entries.  Small MSMs (latency-bound: one wave already saturates a SIMD's integer
// issue, ~10.5 us per mixed addition): 65536 lanes = one wave per SIMD, which halves the number of carries to fold.
// (the shortest chunk: 8 until the short rows' fold became one launch that is linear in the carries per bucket; with it
// 6 is the optimum -- 2^12 row 0.334 -> 0.328 ms, 2^10 0.275 -> 0.268; 4 gives the fold back what the accumulate gains:
// `profiles/r03_ab_min_chunk.log`)
#ifndef KZG_MIN_CHUNK
#define KZG_MIN_CHUNK 6
#endif
int pick_chunk(uint64_t entries) {
    const uint64_t lanes = 131072;
    if (entries <= lanes * 16) {
        const uint64_t k = (entries + lanes / 2 - 1) / (lanes / 2);
        return (int)(k < KZG_MIN_CHUNK ? KZG_MIN_CHUNK : k);
    }
    const uint64_t rounds = (entries + lanes * 512 - 1) / (lanes * 512);
    const uint64_t k = (entries + lanes * rounds - 1) / (lanes * rounds);
    return (int)k;
}
// The bucket tree on stream s: merges level arrays until `stop` nodes are left.  Three buffers in rotation (a level reads its
// own array and the P array of the level below, writes the next) plus a fourth for the two-level launches.  On return b.in is
// the last level array, b.prev the level below it, b.out a buffer nothing reads any more.
struct TreeBufs {
    g1_xyzz_t *in, *prev, *out, *extra;
};
static void run_tree(hipStream_t s, TreeBufs& b, uint32_t n_in, uint32_t stop) {
    for (int level = 0; n_in > stop;) {
        if ((n_in >> 2) >= stop && msm_tree_level2_ok(n_in, level)) {
            // two narrow levels per launch: the level + 1 P array goes to `out`, the level + 2 array to `extra`
            launch_msm_tree_level2(s, b.in, b.prev, b.out, b.extra, n_in, level);
            g1_xyzz_t *old_in = b.in, *old_prev = b.prev;
            b.in = b.extra;
            b.prev = b.out;
            b.out = old_prev;
            b.extra = old_in;
            level += 2;
            n_in >>= 2;
            continue;
        }
        launch_msm_tree_level(s, b.in, b.prev, b.out, n_in, level);
        g1_xyzz_t* recycled = b.prev;
        b.prev = b.in;
        b.in = b.out;
        b.out = recycled;
        level++;
        n_in >>= 1;
    }
}
// ---- the MSM pipeline on device-resident scalars, on lane L: the S = sc.nsets() MSMs of sc's scalar sets over the same n
// points in ONE pass -- set b is sorted into bucket set b, the sort / accumulate / fold / tree kernels simply see S times the
// buckets, the tree stops at S roots and out_xyzz[0 .. S-1] (device, XYZZ) receive the sums.  One kernel sequence, one
// latency-bound tail.  The only host wait inside is on the 4-byte fold-depth read-back; the calling thread holds no lock
// meanwhile.
int msm_core(kzg_ctx* ctx, Lane& L, const ScalarSets& sc, uint64_t n, uint64_t srs_offset, g1_xyzz_t* out_xyzz) {
    hipStream_t s = L.stream;
    const int nbatch = sc.nsets();
    if (sc.nrows < 0 || sc.ntail < 0 || nbatch < 1 || (sc.nrows && !sc.rows) || (sc.ntail && !sc.tail))
        return fail(ctx, KZG_E_ARG, "MSM pass without scalar sets, or with a count and no scalars");
    if (nbatch > std::min(MSM_MAX_SETS, msm_sort_max_sets(ctx->c)))
        return fail(ctx, KZG_E_ARG, "MSM pass with more scalar sets than the sort's key can carry");
    if (n == 0) {
        HIPCHK(ctx, hipMemsetAsync(out_xyzz, 0, nbatch * sizeof(g1_xyzz_t), s));
        return KZG_OK;
    }
    if (srs_offset + n > ctx->stride) return fail(ctx, KZG_E_ARG, "MSM range exceeds the resident SRS");
    const uint64_t entries = n * (uint64_t)ctx->nwin * nbatch;
    if (entries >= ((uint64_t)1 << 32)) return fail(ctx, KZG_E_ARG, "MSM too large for 32-bit entry indices");
    MsmShape sh;
    sh.c = ctx->c; sh.nwin = ctx->nwin; sh.lay = ctx->lay; sh.nbuckets = ctx->nbuckets * nbatch; sh.n = n;
    sh.nbatch = nbatch;
    sh.srs_offset = srs_offset; sh.srs_stride = ctx->stride; sh.chunk = pick_chunk(entries);
    const uint32_t nchunks = (uint32_t)((entries + sh.chunk - 1) / sh.chunk);
    const size_t B = sh.nbuckets;
    L.expect_short = entries <= ((uint64_t)1 << 24);   // up to ~3 ms of GPU time (a 2^20-point MSM)
    L.expect_us += 400 + (uint32_t)(entries / 4096);     // ~0.2 ns per sorted entry + the latency-bound tail
    // Sort mode.  Fast: no count pass, fixed-capacity partition regions -- right for well-spread scalars (field elements
    // of a polynomial), wrong for skewed ones, where a region overflows: that is detected on the device, costs one wasted
    // sort (the queued accumulate sees an empty MSM), and is remembered for the lane's next few calls.
    bool fast = msm_sort_fast_ok(sh) && L.skew_hint == 0;
    if (L.skew_hint > 0) L.skew_hint--;
    HIPCHK(ctx, L.rank.ensure(msm_sort_parted_entries(sh, msm_sort_fast_ok(sh)) * 8));   // partitioned (key_low, value) pairs
    HIPCHK(ctx, L.sorted.ensure(entries * 4));
    HIPCHK(ctx, L.hist.ensure(16384 * 4));
    HIPCHK(ctx, L.offsets.ensure((B + 1) * 4));
    // (+ 16 KB each: whichever buffer is free after the last level also holds the 2 x 32 doubled components of the final)
    HIPCHK(ctx, L.bufA.ensure(B * sizeof(g1_xyzz_t) + 16384));
    HIPCHK(ctx, L.bufB.ensure(B * sizeof(g1_xyzz_t) / 2 + 16384));  // level arrays: n/2^L nodes x L components <= B/2
    HIPCHK(ctx, L.bufC.ensure(B * sizeof(g1_xyzz_t) / 2 + 16384));
    HIPCHK(ctx, L.bufD.ensure((size_t)(LP_MAX_OPS + 64) * sizeof(g1_xyzz_t) + 16384));   // fourth buffer of the two-level launches
    HIPCHK(ctx, L.carries.ensure((size_t)nchunks * sizeof(g1_xyzz_t)));
    HIPCHK(ctx, L.carry_key.ensure((size_t)nchunks * 4));
    uint32_t* max_len_d = L.flags() + 2;
    uint32_t* max_len_h = reinterpret_cast<uint32_t*>(L.pin + PIN_MAXLEN);
    if (nbatch > 2) {   // the final's scratch (nbatch x 32 doubled components) outgrows the 16 KB above on narrow windows
        const size_t fin = (size_t)nbatch * 32 * sizeof(g1_xyzz_t);
        HIPCHK(ctx, L.bufA.ensure(B * sizeof(g1_xyzz_t) + fin));
        HIPCHK(ctx, L.bufB.ensure(B * sizeof(g1_xyzz_t) / 2 + fin));
        HIPCHK(ctx, L.bufC.ensure(B * sizeof(g1_xyzz_t) / 2 + fin));
        HIPCHK(ctx, L.bufD.ensure((size_t)(LP_MAX_OPS + 64) * sizeof(g1_xyzz_t) + fin));
    }
    auto sort_and_publish = [&](bool fast_mode, bool ws_clean) {
        const SortTail tail{(uint32_t)sh.chunk, L.bufA.as<g1_xyzz_t>(), reinterpret_cast<uint32_t*>(L.pin_dev + PIN_MAXLEN),
                            reinterpret_cast<uint32_t*>(L.pin_dev + PIN_SEQ_SORT), ++L.sort_seq};
        launch_msm_sort(s, sh, sc, L.hist.as<uint32_t>(), ws_clean, L.rank.as<uint2>(), L.offsets.as<uint32_t>(),
                        L.sorted.as<uint32_t>(), max_len_d, fast_mode, max_len_d + 1, &tail);
    };
    {
        Span sp(ctx, L, KZG_T_DIGITS);
        // the longest run of carries decides how many fold steps are launched; it depends on the offsets only, so
        // its read-back (with the sort's overflow word) completes while the accumulate kernel runs and costs no bubble.
        // The sort's last kernel takes that maximum, marks the empty buckets and publishes both words itself (SortTail).
        sort_and_publish(fast, L.sort_ws_clean);
        L.sort_ws_clean = true;
        HIPCHK(ctx, hipEventRecord(L.ev_sorted, s));
    }
    {
        Span sp(ctx, L, KZG_T_ACCUMULATE);
        launch_msm_accumulate(s, sh, ctx->table.as<g1_affine_t>(), L.offsets.as<uint32_t>(), L.sorted.as<uint32_t>(),
                              L.bufA.as<g1_xyzz_t>(), L.carries.as<g1_xyzz_t>(), L.carry_key.as<uint32_t>(), nchunks);
    }
    // short rows: the tail's ~20 launches must be queued while the (short) accumulate runs -- poll for the two words
    // instead of sleeping on the event
    auto wait_sorted = [&]() -> hipError_t {
#ifndef KZG_NO_POLL
        if (ctx->profiling != 1 && L.expect_short && poll_pinned(ctx, L, PIN_SEQ_SORT, L.sort_seq)) return hipSuccess;
#endif
        return hipEventSynchronize(L.ev_sorted);
    };
    HIPCHK(ctx, wait_sorted());
    if (fast && max_len_h[1]) {   // a region overflowed: skewed scalars.  Exact sort + accumulate once more.
        L.skew_hint = 16;
        {
            Span sp(ctx, L, KZG_T_DIGITS);
            sort_and_publish(false, true);
            HIPCHK(ctx, hipEventRecord(L.ev_sorted, s));
        }
        {
            Span sp(ctx, L, KZG_T_ACCUMULATE);
            launch_msm_accumulate(s, sh, ctx->table.as<g1_affine_t>(), L.offsets.as<uint32_t>(), L.sorted.as<uint32_t>(),
                                  L.bufA.as<g1_xyzz_t>(), L.carries.as<g1_xyzz_t>(), L.carry_key.as<uint32_t>(), nchunks);
        }
        HIPCHK(ctx, wait_sorted());
    }
    {
        Span sp(ctx, L, KZG_T_FIXUP);
        if (nchunks && msm_fold_bucket_ok(sh.nbuckets, *max_len_h)) {
            launch_fold_bucket(s, L.offsets.as<uint32_t>(), (uint32_t)sh.chunk, sh.nbuckets, L.carries.as<g1_xyzz_t>(),
                               L.bufA.as<g1_xyzz_t>());
        } else {
            for (uint32_t d = 1; d < *max_len_h; d <<= 1)
                launch_fold_step(s, L.offsets.as<uint32_t>(), L.carry_key.as<uint32_t>(), (uint32_t)sh.chunk, nchunks, d,
                                 L.carries.as<g1_xyzz_t>());
            launch_fold_heads(s, L.offsets.as<uint32_t>(), L.carry_key.as<uint32_t>(), (uint32_t)sh.chunk, nchunks,
                              L.carries.as<g1_xyzz_t>(), L.bufA.as<g1_xyzz_t>());
        }
    }
    TreeBufs tb{L.bufA.as<g1_xyzz_t>(), L.bufC.as<g1_xyzz_t>(), L.bufB.as<g1_xyzz_t>(), L.bufD.as<g1_xyzz_t>()};
    {
        Span sp(ctx, L, KZG_T_TREE);
        run_tree(s, tb, sh.nbuckets, (uint32_t)nbatch);
    }
    {
        Span sp(ctx, L, KZG_T_FINAL);
        // `out` (the buffer the last level did not write and no longer reads) holds the doubled components in between
        launch_msm_final(s, tb.in, tb.prev, ctx->c - 1, nbatch, out_xyzz, tb.out);
    }
    HIPCHK(ctx, hipGetLastError());
    return KZG_OK;
}

// twiddle / 1/n tables are shared by all lanes: built once under the ctx mutex, complete before the mutex is dropped
int ensure_twiddles(kzg_ctx* ctx, Lane& L, int log_n, int inverse, uint32_t** tw, uint32_t** invn) {
    std::lock_guard<std::mutex> lk(ctx->mu);
    auto& m = inverse ? ctx->tw_inv : ctx->tw_fwd;
    bool built = false;
    if (log_n >= 1 && !m.count(log_n)) {
        DevBuf b;
        HIPCHK(ctx, b.ensure(((size_t)1 << (log_n - 1)) * 48));   // nine 29-bit limbs per twiddle in a 48-byte slot
        launch_fr_twiddles(L.stream, b.as<uint32_t>(), log_n, inverse);
        m[log_n] = std::move(b);
        built = true;
    }
    *tw = log_n >= 1 ? m[log_n].as<uint32_t>() : nullptr;
    if (invn) {
        if (!ctx->inv_n.count(log_n)) {
            DevBuf b;
            HIPCHK(ctx, b.ensure(32));
            launch_fr_inv_pow2(L.stream, b.as<uint32_t>(), log_n);
            ctx->inv_n[log_n] = std::move(b);
            built = true;
        }
        *invn = ctx->inv_n[log_n].as<uint32_t>();
    }
    if (built) HIPCHK(ctx, hipStreamSynchronize(L.stream));
    return KZG_OK;
}
// coefficients (Montgomery) of the row; returns pointer in *coeffs.  row_dev: Montgomery-form row.
int row_to_coeffs(kzg_ctx* ctx, Lane& L, const uint32_t* row_dev, uint64_t T, int evaluation_form, const uint32_t** coeffs,
                  uint32_t* dst) {   // dst: where the coefficients go instead of the lane's own buffer (row cache)
    if (!evaluation_form || T == 1) {
        if (dst && dst != row_dev) HIPCHK(ctx, hipMemcpyAsync(dst, row_dev, T * 32, hipMemcpyDeviceToDevice, L.stream));
        *coeffs = dst ? dst : row_dev;
        return KZG_OK;
    }
    int lg = ilog2_exact(T);
    if (lg < 0) return fail(ctx, KZG_E_ARG, "evaluation-form row length must be a power of two");
    uint32_t *tw, *invn;
    int rc = ensure_twiddles(ctx, L, lg, 1, &tw, &invn);
    if (rc) return rc;
    if (!dst) {
        HIPCHK(ctx, L.coeffB.ensure(T * 32));
        dst = L.coeffB.as<uint32_t>();
    }
    HIPCHK(ctx, L.ntt_mid.ensure(T * 48));
    Span sp(ctx, L, KZG_T_NTT);
    launch_fr_ntt(L.stream, row_dev, dst, lg, tw, invn, L.ntt_mid.as<uint32_t>());
    *coeffs = dst;
    return KZG_OK;
}
// k rows (k x T elements at rows_dev) in evaluation form: the inverse transform of each into dst (k x T); rows that are
// coefficients already stay where they are
static int rows_to_coeffs(kzg_ctx* ctx, Lane& L, const uint32_t* rows_dev, uint32_t k, uint64_t T, int evaluation_form,
                          uint32_t* dst) {
    for (uint32_t j = 0; evaluation_form && T > 1 && j < k; j++) {
        const uint32_t* c;
        if (int rc = row_to_coeffs(ctx, L, rows_dev + j * T * 8, T, 1, &c, dst + j * T * 8)) return rc;
    }
    return KZG_OK;
}
int check_worker(kzg_ctx* ctx, uint32_t i, uint64_t T) {
    int rc = need_srs(ctx);
    if (rc) return rc;
    if (T == 0) return fail(ctx, KZG_E_ARG, "empty polynomial");
    if (T > ctx->T) return fail(ctx, KZG_E_ARG, "polynomial longer than the worker's SRS slice");
    // (the last resident slice may be shorter than T: a single truncated slice, see plan_table)
    if ((uint64_t)i * ctx->T >= ctx->stride || (uint64_t)i * ctx->T + T > ctx->stride)
        return fail(ctx, KZG_E_ARG, "worker index outside the resident SRS");
    return KZG_OK;
}
// upload BE scalars to `dst` (device limbs); dst must hold n*32 bytes
// the device twin of a staging buffer whose first `bytes` bytes have been flushed (kzg_staging_flush), or null.  The
// caller holds that buffer (it was handed its pointer), so nobody else touches the record meanwhile.
// One-shot: the twin serves the FIRST API call that asks for it (that call may ask more than once: its upload and its
// row-cache verification); any later call finds the flushes forgotten -- the holder may have rewritten the pinned buffer
// between two calls, and a stale twin would be a wrong answer with no error.
const uint8_t* flushed_twin(kzg_ctx* ctx, const uint8_t* host_ptr, uint64_t bytes, hipEvent_t* ev) {
    for (Stage& st : ctx->stage)
        if (host_ptr && st.p_pub.load(std::memory_order_acquire) == host_ptr) {
            if (st.consumed_by && st.consumed_by != call_id_current()) {
                st.flushed = 0;                // a second call on the same held buffer: ordinary upload from the host bytes
                return nullptr;
            }
            if (st.flushed >= bytes && st.flushed && st.twin.p) {
                st.consumed_by = call_id_current();
                *ev = st.ev;
                return static_cast<const uint8_t*>(st.twin.p);
            }
            return nullptr;
        }
    return nullptr;
}
int upload_fr(kzg_ctx* ctx, Lane& L, const uint8_t* be32, uint64_t n, uint32_t* dst, int to_mont) {
    if (!n) return KZG_OK;
    Span sp(ctx, L, KZG_T_DECODE);
    hipEvent_t ev = nullptr;
    if (const uint8_t* twin = flushed_twin(ctx, be32, n * 32, &ev)) {   // uploaded tile by tile while the host decoded
        HIPCHK(ctx, hipStreamWaitEvent(L.stream, ev, 0));
        L.in_be_src = twin;
    } else {
        HIPCHK(ctx, L.in_be.ensure(n * 32));
        HIPCHK(ctx, hipMemcpyAsync(L.in_be.p, be32, n * 32, hipMemcpyHostToDevice, L.stream));
        L.in_be_src = L.in_be.as<uint8_t>();
    }
    launch_fr_from_be(L.stream, L.in_be_src, dst, n, to_mont, L.flags());
    return KZG_OK;
}


// commit and/or open on a device-resident Montgomery row, on the lane(s) the call holds.  With both requested:
//  * rows up to 2^18 (latency-bound: dozens of small dependent kernels): the commitment MSM(U_i, f) and the opening
//    MSM(U_i, q) run as ONE batched pass over the slice's window tables (msm_core with two scalar sets) -- one sort,
//    one accumulate launch, one bucket tree with two roots: a single tail instead of two;
//  * longer rows (throughput-bound): when a second lane is free the opening (evaluation, quotient, MSM) runs there,
//    concurrently with the commitment MSM -- they share only the read-only coefficients -- so that each one's sort and
//    tail hide under the other's accumulate; otherwise (another host thread's request holds the other lanes, or
//    profiling is on) the two MSMs run back to back on this lane and the overlap comes from the other requests.
#ifndef KZG_BATCHED_ROW_MAX
#define KZG_BATCHED_ROW_MAX ((uint64_t)1 << 18)
#endif
int commit_open_dev(kzg_ctx* ctx, LaneHold& H, uint32_t i, const uint32_t* row_dev, uint64_t T, int evaluation_form,
                    const uint8_t* alpha_be32, uint8_t* out_c48, uint8_t* out_eval32, uint8_t* out_p48,
                    const uint32_t* coeffs_ready, uint32_t* coeffs_dst, const VerifyJob* verify) {
    Lane& A = H.L();
    hipStream_t s = A.stream;
    const uint32_t* coeffs = coeffs_ready;     // row cache hit: the coefficient vector is already on the device
    int rc = KZG_OK;
    if (!coeffs) rc = row_to_coeffs(ctx, A, row_dev, T, evaluation_form, &coeffs, coeffs_dst);
    if (rc) return rc;
    const uint64_t offset = (uint64_t)i * ctx->T;
    g1_xyzz_t* res = A.res();
    const bool both = out_c48 && out_p48;
    const bool batched = both && T <= KZG_BATCHED_ROW_MAX;
    Lane* B = (both && !batched) ? H.second() : nullptr;   // lane of the opening, when one is free
    Lane& O = B ? *B : A;
    hipStream_t so = O.stream;
    if (B) {
        HIPCHK(ctx, hipEventRecord(A.ev_coeffs, s));
        HIPCHK(ctx, hipStreamWaitEvent(so, A.ev_coeffs, 0));
    }
    if (out_c48 && !batched) {
        rc = msm_core(ctx, A, ScalarSets::one(coeffs, 1), T, offset, res);
        if (rc) return rc;
    }
    if (out_p48) {
        uint32_t* alpha_m = reinterpret_cast<uint32_t*>(A.tail + TB_ALPHA_M);
        uint32_t* y_m = reinterpret_cast<uint32_t*>(A.tail + TB_Y_M);
        HIPCHK(ctx, O.hbuf.ensure(poly_level_words(T) * 4));
        HIPCHK(ctx, O.hnext.ensure(poly_level_words(T) * 4));
        HIPCHK(ctx, O.qbuf.ensure(T * 32));
        {
            Span sp(ctx, A, KZG_T_POLY, so);
            // alpha rides in as an argument of the opening's first kernel, y leaves big-endian from its scan kernel
            launch_poly_open(so, coeffs, T, alpha_m, O.hbuf.as<uint32_t>(), O.hnext.as<uint32_t>(), y_m,
                             O.qbuf.as<uint32_t>(), alpha_be32, A.flags(), A.tail + TB_EVAL);
        }
        if (batched) {
            // the quotient has T - 1 coefficients; k_poly_quotient leaves a zero in slot T - 1, so it rides as a second
            // length-T scalar set
            rc = msm_core(ctx, A, ScalarSets::rows_tail(coeffs, 1, O.qbuf.as<uint32_t>(), 1, 0), T, offset, res);
        } else {
            rc = msm_core(ctx, O, ScalarSets::one(O.qbuf.as<uint32_t>(), 0), T - 1, offset, res + 1);
        }
        if (rc) return rc;
        if (B) {
            HIPCHK(ctx, hipEventRecord(B->ev_done, so));
            HIPCHK(ctx, hipStreamWaitEvent(s, B->ev_done, 0));
        }
    }
    queue_encode(ctx, A, out_c48 != nullptr, out_p48 != nullptr);
    if (verify) {   // row-cache hit: queued LAST, so that its few runtime calls cost host time while the GPU is busy with the
        // request's own kernels; the copy and the comparison run beside them, the publish waits for the verdict
        uint32_t* vflag = reinterpret_cast<uint32_t*>(A.tail + TB_VERIFY);
        HIPCHK(ctx, hipMemsetAsync(vflag, 0, 4, A.vstream));
        hipEvent_t fev = nullptr;
        const uint32_t* mine = reinterpret_cast<const uint32_t*>(flushed_twin(ctx, verify->row_be32, verify->T * 32, &fev));
        if (mine) {      // the row is already on the device (flushed tile by tile during the decode)
            HIPCHK(ctx, hipStreamWaitEvent(A.vstream, fev, 0));
        } else {
            HIPCHK(ctx, A.vbuf.ensure(verify->T * 32));
            HIPCHK(ctx, hipMemcpyAsync(A.vbuf.p, verify->row_be32, verify->T * 32, hipMemcpyHostToDevice, A.vstream));
            mine = A.vbuf.as<uint32_t>();
        }
        launch_words_differ(A.vstream, mine, verify->cached_raw, verify->T * 8, vflag);
        HIPCHK(ctx, hipEventRecord(A.ev_verify, A.vstream));
        HIPCHK(ctx, hipStreamWaitEvent(s, A.ev_verify, 0));   // the record must carry TB_VERIFY's final value
    }
    rc = finish(ctx, A);
    if (rc) return rc;
    if (out_c48 && out_p48 && ctx->host_finish)     // both points, one shared inversion
        kzg_host::xyzz_pair_to_c48(reinterpret_cast<const uint32_t*>(A.pin + TB_RES0),
                                   reinterpret_cast<const uint32_t*>(A.pin + TB_RES1), out_c48, out_p48);
    else {
        if (out_c48) result_c48(ctx, A, 0, out_c48);
        if (out_p48) result_c48(ctx, A, 1, out_p48);
    }
    if (out_p48) memcpy(out_eval32, A.pin + TB_EVAL, 32);
    H.clean = true;
    return KZG_OK;
}


// ---- the back half of every multi-row call: k row sets + m quotient sets -> passes of msm_core -> the record -> the host.

// the multi-row record (MR_*) and its pinned page, allocated by the first multi-row call on the lane
static int ensure_multi_record(kzg_ctx* ctx, Lane& A) {
    HIPCHK(ctx, A.brec.ensure(MR_SIZE));
    if (!A.bpin) {
        uint8_t* p = nullptr;
        HIPCHK(ctx, hipHostMalloc((void**)&p, 8192, hipHostMallocMapped | hipHostMallocCoherent));
        A.bpin = p;
        HIPCHK(ctx, hipHostGetDevicePointer((void**)&A.bpin_dev, A.bpin, 0));
    }
    return KZG_OK;
}
#ifndef KZG_BATCH_PASS_SETS
#define KZG_BATCH_PASS_SETS MSM_MAX_SETS   // (A/B knob: a smaller cap splits a batch into more passes)
#endif
// Sets 0 .. k-1 are the rows, k .. k+m-1 the quotients; consecutive sets share a pass.
//  * rows up to KZG_BATCHED_ROW_MAX (latency-bound): as many sets per pass as the sort's key carries (msm_sort_max_sets);
//    bucket memory caps a pass of more than two sets at 2^22 buckets;
//  * longer rows (throughput-bound: a multi-set pass there only adds buckets to a sort that is no longer latency): one set
//    per pass, alternating between the call's lane and a second one (when one is free), as commit_open_dev spreads its two.
uint32_t plan_msm_passes(int c, uint32_t nbuckets, bool long_rows, uint32_t k, uint32_t m, MsmPass* out) {
    uint32_t per = (uint32_t)std::min(KZG_BATCH_PASS_SETS, msm_sort_max_sets(c));
    while (per > 2 && (uint64_t)per * nbuckets > ((uint64_t)1 << 22)) per--;
    if (long_rows) per = 1;
    uint32_t passes = 0;
    for (uint32_t a = 0; a < k + m; a += per, passes++) {
        const uint32_t b = std::min(k + m, a + per), ra = std::min(a, k), rb = std::min(b, k);
        out[passes] = MsmPass{ra, rb - ra, a - ra, (b - a) - (rb - ra), long_rows ? passes & 1u : 0u};
    }
    return passes;
}
// the MSMs over U_i and the end of a multi-row call: the k rows (Montgomery, consecutive at coef) and the m quotients in
// A.qbuf, in the passes of plan_msm_passes.  Writes the k commitments, the npairs evaluations of the record and the m proofs
// (each output unused when its count is 0).
static int multi_msms_finish(kzg_ctx* ctx, LaneHold& H, uint32_t i, uint64_t T, const uint32_t* coef, uint32_t k,
                             uint32_t m, uint32_t npairs, uint8_t* out_c48, uint8_t* out_evals32, uint8_t* out_p48) {
    Lane& A = H.L();
    hipStream_t s = A.stream;
    const uint64_t words = T * 8;   // one row, in words
    uint8_t* rec = A.brec.as<uint8_t>();
    g1_xyzz_t* res = reinterpret_cast<g1_xyzz_t*>(rec + MR_RES);
    const uint32_t* q = A.qbuf.as<uint32_t>();
    MsmPass pass[MR_SETS];
    const uint32_t sets = k + m, passes = plan_msm_passes(ctx->c, ctx->nbuckets, T > KZG_BATCHED_ROW_MAX, k, m, pass);
    Lane* B = (passes > 1 && pass[1].lane) ? H.second() : nullptr;
    if (B) {
        HIPCHK(ctx, hipEventRecord(A.ev_coeffs, s));
        HIPCHK(ctx, hipStreamWaitEvent(B->stream, A.ev_coeffs, 0));
    }
    for (uint32_t p = 0; p < passes; p++) {
        const MsmPass& P = pass[p];
        const ScalarSets sc = ScalarSets::rows_tail(P.nrows ? coef + P.row0 * words : nullptr, (int)P.nrows,
                                                    P.ntail ? q + P.tail0 * words : nullptr, (int)P.ntail, words);
        if (int rc = msm_core(ctx, (B && P.lane) ? *B : A, sc, T, (uint64_t)i * ctx->T, res + P.row0 + P.tail0)) return rc;
    }
    if (B) {
        HIPCHK(ctx, hipEventRecord(B->ev_done, B->stream));
        HIPCHK(ctx, hipStreamWaitEvent(s, B->ev_done, 0));
    }
    if (!ctx->host_finish) {
        Span sp(ctx, A, KZG_T_FINAL);
        for (uint32_t p = 0; p + 1 < sets; p += 2)
            launch_g1_compress_pair(s, res + p, res + p + 1, rec + MR_C48 + 48 * p, rec + MR_C48 + 48 * (p + 1));
        if (sets & 1) launch_g1_compress(s, res + sets - 1, rec + MR_C48 + 48 * (sets - 1));
    }
    launch_publish(s, rec, A.bpin_dev, MR_COPY);   // stream-ordered ahead of finish()'s record and its sequence word
    int rc = finish(ctx, A);
    if (rc) return rc;
    if (ctx->host_finish) {
        uint8_t enc[MR_SETS * 48];
        kzg_host::xyzz_batch_to_c48(reinterpret_cast<const uint32_t*>(A.bpin + MR_RES), sets, enc);
        if (k) memcpy(out_c48, enc, 48 * (size_t)k);
        if (m) memcpy(out_p48, enc + 48 * (size_t)k, 48 * (size_t)m);
    } else {
        if (k) memcpy(out_c48, A.bpin + MR_C48, 48 * (size_t)k);
        if (m) memcpy(out_p48, A.bpin + MR_C48 + 48 * (size_t)k, 48 * (size_t)m);
    }
    if (npairs) memcpy(out_evals32, A.bpin + MR_EVAL, 32 * (size_t)npairs);
    H.clean = true;
    return KZG_OK;
}

// ---- the batched opening (kzg_commit_open_batch): k rows f_j of worker i, one point alpha, one challenge gamma.
//   INTT of each row -> the k evaluations y_j = f_j(alpha) side by side (launch_poly_eval_rows: the launches of ONE
//   evaluation) -> h = sum_j gamma^j f_j (launch_fr_combine_rows) -> the opening of h (launch_poly_open: its quotient
//   lands in the proof's scalar set) -> the k + 1 MSMs over the slice U_i (multi_msms_finish with one quotient): one pass
//   for short rows while the window leaves the sort's key room, k + 1 MSMs where k single-row calls run 2k.
int commit_open_batch_dev(kzg_ctx* ctx, LaneHold& H, uint32_t i, const uint32_t* rows_dev, uint32_t k, uint64_t T,
                          int evaluation_form, const uint8_t* alpha_be32, const uint8_t* gamma_be32, uint8_t* out_c48,
                          uint8_t* out_evals32, uint8_t* out_p48) {
    Lane& A = H.L();
    hipStream_t s = A.stream;
    if (int rc = ensure_multi_record(ctx, A)) return rc;
    const bool intt = evaluation_form && T > 1;
    if (intt) HIPCHK(ctx, A.bcoef.ensure(k * T * 32));
    const uint32_t* coef = intt ? A.bcoef.as<uint32_t>() : rows_dev;
    if (int rc = rows_to_coeffs(ctx, A, rows_dev, k, T, evaluation_form, A.bcoef.as<uint32_t>())) return rc;
    uint8_t* rec = A.brec.as<uint8_t>();   // (alpha and y of the combination's opening: the lane's own tail record)
    uint32_t* alpha_m = reinterpret_cast<uint32_t*>(A.tail + TB_ALPHA_M);
    uint32_t* y_m = reinterpret_cast<uint32_t*>(A.tail + TB_Y_M);
    const uint64_t hrow = poly_level_words(T);   // level scratch of one row
    HIPCHK(ctx, A.hbuf.ensure(k * hrow * 4));
    HIPCHK(ctx, A.hnext.ensure(k * hrow * 4));
    HIPCHK(ctx, A.bcomb.ensure(T * 32));
    HIPCHK(ctx, A.qbuf.ensure(T * 32));
    uint32_t* hcomb = A.bcomb.as<uint32_t>();
    uint32_t* q = A.qbuf.as<uint32_t>();
    {
        Span sp(ctx, A, KZG_T_POLY);
        // alpha rides in as an argument of the evaluations' first kernel, gamma as one of the combination's
        launch_poly_eval_rows(s, coef, T, k, alpha_m, A.hbuf.as<uint32_t>(), A.hnext.as<uint32_t>(), hrow,
                              reinterpret_cast<uint32_t*>(rec + MR_Y_M), alpha_be32, A.flags(), rec + MR_EVAL);
        launch_fr_combine_rows(s, coef, T, k, gamma_be32, hcomb, A.flags());
        // k_poly_quotient leaves a zero in slot T - 1: the quotient rides as one more length-T scalar set
        launch_poly_open(s, hcomb, T, alpha_m, A.hbuf.as<uint32_t>(), A.hnext.as<uint32_t>(), y_m, q);
    }
    return multi_msms_finish(ctx, H, i, T, coef, k, 1, k, out_c48, out_evals32, out_p48);
}

// ---- the multi-point opening (kzg_commit_open_multi): k rows f_j of worker i, m points alpha_p, point p opening the rows of
// masks[p] with its own challenge gamma_p.
//   INTT of each row (once) -> every masked (row, point) pair evaluated side by side (launch_poly_eval_pairs: the launches
//   of ONE evaluation; rows past KZG_BATCHED_ROW_MAX in groups of KZG_MAX_BATCH_OPEN pairs, whose level scratch is large)
//   -> the m combinations h_p in one launch (launch_fr_combine_points) -> their m openings side by side
//   (launch_poly_open_points: the quotients land in m consecutive length-T scalar sets) -> the k + m MSMs over U_i
//   (multi_msms_finish: one pass while the sort's key and 2^22 buckets allow).
// The committed row sets (kzg_rows_commit / kzg_rows_open) run the two halves of the same sequence: the commit its INTT and
// k MSMs, the open its pairs, combinations, quotients and m MSMs, reading the rows through the same table of row pointers.

// the masked (row, point) pairs of nrows rows at m points, point-major, ascending rows inside a point (the order of
// out_evals32), with the points as the evaluations' kernel argument; rows past KZG_BATCHED_ROW_MAX are evaluated in groups
// of KZG_MAX_BATCH_OPEN pairs (their level scratch is large)
struct PairPlan {
    PairArg pa;
    uint32_t npairs, group;
    uint64_t hrow;   // level scratch of one pair (or one point's combination), words
};
static void plan_pairs(PairPlan& pp, uint32_t nrows, uint64_t T, uint32_t m, const uint8_t* points_be32,
                       const uint32_t* masks) {
    memset(&pp.pa, 0, sizeof(pp.pa));
    pp.npairs = 0;
    for (uint32_t p = 0; p < m; p++) {
        memcpy(pp.pa.a[p].w, points_be32 + 32 * (size_t)p, 32);
        for (uint32_t j = 0; j < nrows; j++)
            if ((masks[p] >> j) & 1u) {
                pp.pa.row[pp.npairs] = (uint8_t)j;
                pp.pa.pt[pp.npairs++] = (uint8_t)p;
            }
    }
    pp.hrow = poly_level_words(T);
    pp.group = T <= KZG_BATCHED_ROW_MAX ? pp.npairs : std::min<uint32_t>(pp.npairs, KZG_MAX_BATCH_OPEN);
}
// every pair evaluated (rows read at rt.r[j]): the evaluations land in the record (MR_EVAL big-endian, MR_Y_M Montgomery),
// the points' Montgomery forms at MR_ALPHA_M.  The lane's level scratch must hold pp.group pairs.
static void launch_pairs(Lane& A, const RowTab& rt, uint64_t T, const PairPlan& pp) {
    uint8_t* rec = A.brec.as<uint8_t>();
    uint32_t* alpha_m = reinterpret_cast<uint32_t*>(rec + MR_ALPHA_M);
    for (uint32_t g0 = 0; g0 < pp.npairs; g0 += pp.group) {   // the points ride in as arguments of each group's first kernel
        const uint32_t ng = std::min(pp.group, pp.npairs - g0);
        PairArg ga = pp.pa;
        memmove(ga.row, pp.pa.row + g0, ng);
        memmove(ga.pt, pp.pa.pt + g0, ng);
        launch_poly_eval_pairs(A.stream, rt, T, ng, ga, alpha_m, A.hbuf.as<uint32_t>(), A.hnext.as<uint32_t>(), pp.hrow,
                               reinterpret_cast<uint32_t*>(rec + MR_Y_M) + 8 * g0, A.flags(), rec + MR_EVAL + 32 * g0);
    }
}
// the openings of nrows rows (row j's Montgomery coefficients at rt.r[j]) at m points: the pairs' evaluations land in the
// record (MR_EVAL, point-major), the m quotients in A.qbuf as m consecutive length-T canonical scalar sets
static int multi_open_poly(kzg_ctx* ctx, Lane& A, const RowTab& rt, uint32_t nrows, uint64_t T, uint32_t m,
                           const uint8_t* points_be32, const uint32_t* masks, const uint8_t* gammas_be32, uint32_t* out_npairs) {
    hipStream_t s = A.stream;
    PairPlan pp;
    plan_pairs(pp, nrows, T, m, points_be32, masks);
    CombArg ca;
    memset(&ca, 0, sizeof(ca));
    for (uint32_t p = 0; p < m; p++) {
        memcpy(ca.g[p].w, gammas_be32 + 32 * (size_t)p, 32);
        ca.mask[p] = masks[p];
    }
    uint8_t* rec = A.brec.as<uint8_t>();
    uint32_t* alpha_m = reinterpret_cast<uint32_t*>(rec + MR_ALPHA_M);
    const uint64_t hrow = pp.hrow;
    HIPCHK(ctx, A.hbuf.ensure(std::max(pp.group, m) * hrow * 4));
    HIPCHK(ctx, A.hnext.ensure(std::max(pp.group, m) * hrow * 4));
    HIPCHK(ctx, A.bcomb.ensure(m * T * 32));
    HIPCHK(ctx, A.qbuf.ensure(m * T * 32));
    uint32_t* hcomb = A.bcomb.as<uint32_t>();
    const uint32_t npairs = pp.npairs;
    Span sp(ctx, A, KZG_T_POLY);
    launch_pairs(A, rt, T, pp);
    launch_fr_combine_points(s, rt, T, m, ca, hcomb, A.flags());
    // k_poly_quotient leaves a zero in slot T - 1: each quotient rides as one more length-T scalar set
    launch_poly_open_points(s, hcomb, T, m, alpha_m, A.hbuf.as<uint32_t>(), A.hnext.as<uint32_t>(), hrow,
                            reinterpret_cast<uint32_t*>(rec + MR_HY_M), A.qbuf.as<uint32_t>());
    *out_npairs = npairs;
    return KZG_OK;
}
int commit_open_multi_dev(kzg_ctx* ctx, LaneHold& H, uint32_t i, const uint32_t* rows_dev, uint32_t k, uint64_t T,
                          int evaluation_form, uint32_t m, const uint8_t* points_be32, const uint32_t* masks,
                          const uint8_t* gammas_be32, uint8_t* out_c48, uint8_t* out_evals32, uint8_t* out_p48) {
    Lane& A = H.L();
    if (int rc = ensure_multi_record(ctx, A)) return rc;
    const bool intt = evaluation_form && T > 1;
    if (intt) HIPCHK(ctx, A.bcoef.ensure(k * T * 32));
    const uint32_t* coef = intt ? A.bcoef.as<uint32_t>() : rows_dev;
    if (int rc = rows_to_coeffs(ctx, A, rows_dev, k, T, evaluation_form, A.bcoef.as<uint32_t>())) return rc;
    RowTab rt;
    memset(&rt, 0, sizeof(rt));
    for (uint32_t j = 0; j < k; j++) rt.r[j] = coef + j * T * 8;
    uint32_t npairs = 0;
    if (int rc = multi_open_poly(ctx, A, rt, k, T, m, points_be32, masks, gammas_be32, &npairs)) return rc;
    return multi_msms_finish(ctx, H, i, T, coef, k, m, npairs, out_c48, out_evals32, out_p48);
}

// ---- committed row sets.  The commit: rows (Montgomery, k x T at rows_dev) -> their coefficients in the set's own buffer
// `dst` (the INTT writes there; coefficient-form rows were uploaded there already) -> the k commitment MSMs.
int rows_commit_dev(kzg_ctx* ctx, LaneHold& H, uint32_t i, const uint32_t* rows_dev, uint32_t k, uint64_t T,
                    int evaluation_form, uint32_t* dst, uint8_t* out_c48) {
    Lane& A = H.L();
    if (int rc = ensure_multi_record(ctx, A)) return rc;
    if (int rc = rows_to_coeffs(ctx, A, rows_dev, k, T, evaluation_form, dst)) return rc;
    return multi_msms_finish(ctx, H, i, T, dst, k, 0, 0, out_c48, nullptr, nullptr);
}
// The open: the coefficient rows of committed sets (row j at rt.r[j], read in place) at m points -> the m proofs.
int rows_open_dev(kzg_ctx* ctx, LaneHold& H, uint32_t i, const RowTab& rt, uint32_t k, uint64_t T, uint32_t m,
                  const uint8_t* points_be32, const uint32_t* masks, const uint8_t* gammas_be32, uint8_t* out_evals32,
                  uint8_t* out_p48) {
    Lane& A = H.L();
    if (int rc = ensure_multi_record(ctx, A)) return rc;
    uint32_t npairs = 0;
    if (int rc = multi_open_poly(ctx, A, rt, k, T, m, points_be32, masks, gammas_be32, &npairs)) return rc;
    return multi_msms_finish(ctx, H, i, T, nullptr, 0, m, npairs, nullptr, out_evals32, out_p48);
}
// The evaluations alone (kzg_rows_eval): the open's pair evaluations, then the record -- no combination, no quotient, no MSM.
int rows_eval_dev(kzg_ctx* ctx, LaneHold& H, uint32_t i, const RowTab& rt, uint32_t k, uint64_t T, uint32_t m,
                  const uint8_t* points_be32, const uint32_t* masks, uint8_t* out_evals32) {
    Lane& A = H.L();
    if (int rc = ensure_multi_record(ctx, A)) return rc;
    PairPlan pp;
    plan_pairs(pp, k, T, m, points_be32, masks);
    HIPCHK(ctx, A.hbuf.ensure(pp.group * pp.hrow * 4));
    HIPCHK(ctx, A.hnext.ensure(pp.group * pp.hrow * 4));
    {
        Span sp(ctx, A, KZG_T_POLY);
        launch_pairs(A, rt, T, pp);
    }
    A.expect_short = true;   // a few scans, no MSM: finish() may poll for the record
    return multi_msms_finish(ctx, H, i, T, nullptr, 0, 0, pp.npairs, nullptr, out_evals32, nullptr);
}
// The caller-weighted openings (kzg_rows_open_lincomb): the m combinations h_p = sum_j lambda_{p,j} f_j in one launch
// (k_fr_lincomb_points, which also converts the points), their m openings side by side -- v_p = h_p(alpha_p) leaves the
// quotient scan big-endian in the MR_EVAL slots, which no pair uses here -- and the m quotient MSMs.  No pair evaluation,
// no commitment MSM.
int rows_lincomb_dev(kzg_ctx* ctx, LaneHold& H, uint32_t i, const RowTab& rt, uint32_t k, uint64_t T, uint32_t m,
                     const uint8_t* points_be32, const uint8_t* coeffs_be32, const uint32_t* masks, uint8_t* out_values32,
                     uint8_t* out_p48) {
    Lane& A = H.L();
    if (int rc = ensure_multi_record(ctx, A)) return rc;
    uint8_t* rec = A.brec.as<uint8_t>();
    uint32_t* alpha_m = reinterpret_cast<uint32_t*>(rec + MR_ALPHA_M);
    const uint64_t hrow = poly_level_words(T);   // level scratch of one point's combination
    HIPCHK(ctx, A.hbuf.ensure(m * hrow * 4));
    HIPCHK(ctx, A.hnext.ensure(m * hrow * 4));
    HIPCHK(ctx, A.bcomb.ensure(m * T * 32));
    HIPCHK(ctx, A.qbuf.ensure(m * T * 32));
    uint32_t* hcomb = A.bcomb.as<uint32_t>();
    {
        Span sp(ctx, A, KZG_T_POLY);
        launch_fr_lincomb_points(A.stream, rt, T, m, k, coeffs_be32, masks, points_be32, hcomb, alpha_m, A.flags());
        launch_poly_open_points(A.stream, hcomb, T, m, alpha_m, A.hbuf.as<uint32_t>(), A.hnext.as<uint32_t>(), hrow,
                                reinterpret_cast<uint32_t*>(rec + MR_HY_M), A.qbuf.as<uint32_t>(), rec + MR_EVAL);
    }
    return multi_msms_finish(ctx, H, i, T, nullptr, 0, m, m, nullptr, out_values32, out_p48);
}
// The first SHPLONK round (kzg_rows_commit_shplonk): a set built FROM sets.  h = sum_S quot(g_S, Z_S) over the groups of rows
// with one point set S, g_S = sum_{j in group} c_j f_j.  Groups run in batches of at most KZG_MAX_OPEN_POINTS: one launch
// combines the batch's g_S (k_fr_lincomb_points, "point" read as "group"), then pass d divides every group that still has a
// d-th point by (X - that point) -- the launches of ONE opening, grid y = group, the quotient kept in Montgomery form -- the
// vectors going back and forth between the two lane buffers of the caller-weighted opening; one launch adds the batch's final
// quotients into the new set's buffer `dst`; one MSM commits.  The remainders are never looked at: dividing on by the next
// point drops them.  Workspace: what rows_lincomb_dev holds at m = KZG_MAX_OPEN_POINTS, whatever the number of groups.
int rows_shplonk_dev(kzg_ctx* ctx, LaneHold& H, uint32_t i, const RowTab& rt, uint32_t k, uint64_t T, uint32_t m,
                     const uint8_t* points_be32, const uint8_t* coeffs_be32, uint32_t n_groups, const ShGroup* groups,
                     uint32_t* dst, uint8_t* out_c48) {
    Lane& A = H.L();
    if (int rc = ensure_multi_record(ctx, A)) return rc;
    hipStream_t s = A.stream;
    uint8_t* rec = A.brec.as<uint8_t>();
    uint32_t* alpha_m = reinterpret_cast<uint32_t*>(rec + MR_SH_ALPHA_M);
    const uint32_t B = KZG_MAX_OPEN_POINTS;   // groups per batch
    static_assert(KZG_MAX_OPEN_POINTS <= POLY_MAX_POINTS && KZG_MAX_OPEN_POINTS <= POLY_MAX_ROWS,
                  "a batch is one launch of the combination, of each division and of the sum");
    const uint64_t words = T * 8;
    const uint64_t hrow = poly_level_words(T);   // level scratch of one group's division
    HIPCHK(ctx, A.hbuf.ensure(B * hrow * 4));
    HIPCHK(ctx, A.hnext.ensure(B * hrow * 4));
    HIPCHK(ctx, A.bcomb.ensure(B * T * 32));
    HIPCHK(ctx, A.qbuf.ensure(B * T * 32));
    {
        Span sp(ctx, A, KZG_T_POLY);
        for (uint32_t p = 0; p < m; p++) launch_fr_from_host32(s, points_be32 + 32 * (size_t)p, alpha_m + 8 * p, 1, A.flags());
        for (uint32_t g0 = 0; g0 < n_groups; g0 += B) {
            const uint32_t G = std::min(B, n_groups - g0);
            uint8_t lam[KZG_MAX_OPEN_POINTS * KZG_MAX_BATCH_OPEN * 32] = {};   // group-major: c_j on the group's rows
            uint32_t masks[KZG_MAX_OPEN_POINTS] = {};
            for (uint32_t g = 0; g < G; g++) {
                masks[g] = groups[g0 + g].rows;
                for (uint32_t j = 0; j < k; j++)
                    if ((masks[g] >> j) & 1u) memcpy(lam + 32 * ((size_t)g * k + j), coeffs_be32 + 32 * (size_t)j, 32);
            }
            uint32_t *cur = A.bcomb.as<uint32_t>(), *nxt = A.qbuf.as<uint32_t>();
            launch_fr_lincomb_points(s, rt, T, G, k, lam, masks, nullptr, cur, nullptr, A.flags());
            RowTab fin;   // where each group's last quotient lies
            memset(&fin, 0, sizeof(fin));
            for (uint32_t d = 0; d < groups[g0].npts; d++) {   // (descending npts: the groups with a d-th point are a prefix)
                uint32_t nact = 0;
                uint8_t pts[KZG_MAX_OPEN_POINTS] = {};
                while (nact < G && groups[g0 + nact].npts > d) {
                    pts[nact] = groups[g0 + nact].pt[d];
                    nact++;
                }
                launch_poly_open_points(s, cur, T, nact, alpha_m, A.hbuf.as<uint32_t>(), A.hnext.as<uint32_t>(), hrow,
                                        reinterpret_cast<uint32_t*>(rec + MR_HY_M), nxt, nullptr, pts, true);
                for (uint32_t g = 0; g < nact; g++)
                    if (groups[g0 + g].npts == d + 1) fin.r[g] = nxt + g * words;
                std::swap(cur, nxt);
            }
            launch_fr_sum_rows(s, fin, G, T, g0 != 0, dst);
        }
    }
    return multi_msms_finish(ctx, H, i, T, dst, 1, 0, 0, out_c48, nullptr, nullptr);
}
// The back half of a grand product, the permutation's and the shuffle's alike: the running vectors N and D (T factors each,
// in the lane's bcomb / qbuf) become z's evaluations through the product scans and the one inversion (fr_prod.hip); the inverse
// transform writes z's coefficients straight into the new set's buffer `dst`; one MSM commits.  The record's first two
// evaluation slots carry the closing value and the zero-denominator flag word.
static int grand_product_finish_dev(kzg_ctx* ctx, LaneHold& H, uint32_t i, uint32_t* N, uint32_t* D, uint64_t T, uint32_t* dst,
                                    uint8_t* out_c48, uint8_t* out_closing32, bool* out_zero_den, const Blind* zk,
                                    const uint8_t* start_be32) {
    Lane& A = H.L();
    uint8_t* rec = A.brec.as<uint8_t>();
    {
        Span sp(ctx, A, KZG_T_POLY);
        // _zk: N_t = D_t = 1 on the rows >= usable (whatever their cells hold, a zero D_t included), so the unchanged scan
        // leaves z = closing on every one of them; the tail then replaces the rows behind row `usable`
        if (zk) launch_blind_mask(A.stream, N, true, D, T, zk->usable);
        // _chain: start_be32 is folded into the scan's top-level prefix values: every row and the closing value carry it, and
        // the tail below overwrites the rows behind row `usable`
        launch_gp_scan(A.stream, N, D, T, A.hbuf.as<uint32_t>(), A.hnext.as<uint32_t>(), rec + MR_EVAL,
                       reinterpret_cast<uint32_t*>(rec + MR_EVAL + 32), start_be32);
        if (zk) launch_blind_tail(A.stream, N, T, zk->usable, zk->tail_be32, A.flags());
    }
    const uint32_t* c;
    if (int rc = row_to_coeffs(ctx, A, N, T, 1, &c, dst)) return rc;
    uint8_t ev[64];
    if (int rc = multi_msms_finish(ctx, H, i, T, dst, 1, 0, 2, out_c48, ev, nullptr)) return rc;
    memcpy(out_closing32, ev, 32);
    uint32_t zf;
    memcpy(&zf, ev + 32, 4);
    *out_zero_den = zf != 0;
    return KZG_OK;
}
// The permutation grand product (kzg_rows_commit_grand_product): a set built FROM sets.  Per wire / sigma pair two forward
// transforms of the sets' coefficient rows into two lane buffers and one launch that folds the pair's factors into the
// running N and D vectors (four vectors of T whatever k is); the product scans and the one inversion turn N into z's
// evaluations (fr_prod.hip); the inverse transform writes z's coefficients straight into the new set's buffer `dst`; one
// MSM commits.  The record's first two evaluation slots carry the closing value and the zero-denominator flag word.
int rows_grand_product_dev(kzg_ctx* ctx, LaneHold& H, uint32_t i, const RowTab& wires, const RowTab& sigmas, uint32_t k,
                           uint64_t T, const uint8_t* shifts_be32, const uint8_t* beta_be32, const uint8_t* gamma_be32,
                           uint32_t* dst, uint8_t* out_c48, uint8_t* out_closing32, bool* out_zero_den, const Blind* zk,
                           const uint8_t* start_be32) {
    Lane& A = H.L();
    if (int rc = ensure_multi_record(ctx, A)) return rc;
    const int lg = ilog2_exact(T);
    uint32_t* tw = nullptr;
    if (int rc = ensure_twiddles(ctx, A, lg, 0, &tw, nullptr)) return rc;
    HIPCHK(ctx, A.coeffA.ensure(T * 32));
    HIPCHK(ctx, A.coeffB.ensure(T * 32));
    HIPCHK(ctx, A.bcomb.ensure(T * 32));
    HIPCHK(ctx, A.qbuf.ensure(T * 32));
    HIPCHK(ctx, A.ntt_mid.ensure(T * 48));
    HIPCHK(ctx, A.hbuf.ensure(poly_level_words(T) * 4));
    HIPCHK(ctx, A.hnext.ensure(poly_level_words(T) * 4));
    uint32_t *ea = A.coeffA.as<uint32_t>(), *es = A.coeffB.as<uint32_t>();
    uint32_t *N = A.bcomb.as<uint32_t>(), *D = A.qbuf.as<uint32_t>();
    for (uint32_t j = 0; j < k; j++) {
        {
            Span sp(ctx, A, KZG_T_NTT);
            launch_fr_ntt(A.stream, wires.r[j], ea, lg, tw, nullptr, A.ntt_mid.as<uint32_t>());
            launch_fr_ntt(A.stream, sigmas.r[j], es, lg, tw, nullptr, A.ntt_mid.as<uint32_t>());
        }
        Span sp(ctx, A, KZG_T_POLY);
        launch_gp_factors(A.stream, ea, es, N, D, T, tw, beta_be32, gamma_be32, shifts_be32 + 32 * (size_t)j, j == 0, A.flags());
    }
    return grand_product_finish_dev(ctx, H, i, N, D, T, dst, out_c48, out_closing32, out_zero_den, zk, start_be32);
}

// The shuffle grand product (kzg_rows_commit_shuffle): a set built FROM sets.  Per group, the input side and then the shuffle
// side: every row of the side is transformed into ONE lane buffer and folded in as it arrives, by Horner in theta from the last
// column down (fr_lookup.hip's LK_HORNER); column 0 closes the chain with k_sh_factor, which multiplies gamma + A_g (or the
// selected form) into N, gamma + B_g into D.  A side's selector row is transformed into one further vector just in front of
// that launch (kept when the next side names the same row).  Workspace: the grand product's four vectors of T (the
// transform's output, the Horner accumulator, N, D) and its scan scratch, plus one vector of T when a selector is named --
// whatever n_groups and width are.  From N and D on, the call is the grand product's.
int rows_shuffle_dev(kzg_ctx* ctx, LaneHold& H, uint32_t i, const RowTab& inputs, const RowTab& shuffles, uint32_t n_groups,
                     uint32_t width, uint64_t T, const uint8_t* theta_be32, const uint8_t* gamma_be32, uint32_t* dst,
                     uint8_t* out_c48, uint8_t* out_closing32, bool* out_zero_den, const Blind* zk, const ShuffleSel* sel) {
    Lane& A = H.L();
    if (int rc = ensure_multi_record(ctx, A)) return rc;
    const int lg = ilog2_exact(T);
    uint32_t* tw = nullptr;
    if (int rc = ensure_twiddles(ctx, A, lg, 0, &tw, nullptr)) return rc;
    HIPCHK(ctx, A.coeffA.ensure(T * 32));
    HIPCHK(ctx, A.coeffB.ensure(T * 32));
    HIPCHK(ctx, A.bcomb.ensure(T * 32));
    HIPCHK(ctx, A.qbuf.ensure(T * 32));
    HIPCHK(ctx, A.ntt_mid.ensure(T * 48));
    HIPCHK(ctx, A.hbuf.ensure(poly_level_words(T) * 4));
    HIPCHK(ctx, A.hnext.ensure(poly_level_words(T) * 4));
    if (sel) HIPCHK(ctx, A.qext.ensure(T * 32));
    uint32_t *e = A.coeffA.as<uint32_t>(), *acc = A.coeffB.as<uint32_t>(), *mid = A.ntt_mid.as<uint32_t>();
    uint32_t *N = A.bcomb.as<uint32_t>(), *D = A.qbuf.as<uint32_t>();
    const uint32_t* sel_in_q = nullptr;   // the selector row whose evaluations lie in qext
    for (uint32_t g = 0; g < n_groups; g++) {
        for (int side = 0; side < 2; side++) {
            const RowTab& rt = side ? shuffles : inputs;
            const uint32_t* q = sel ? (side ? sel->sh[g] : sel->in[g]) : nullptr;
            for (uint32_t c = width; c-- > 0;) {
                {
                    Span sp(ctx, A, KZG_T_NTT);
                    launch_fr_ntt(A.stream, rt.r[g * width + c], e, lg, tw, nullptr, mid);
                    if (!c && q && q != sel_in_q) {
                        launch_fr_ntt(A.stream, q, A.qext.as<uint32_t>(), lg, tw, nullptr, mid);
                        sel_in_q = q;
                    }
                }
                Span sp(ctx, A, KZG_T_POLY);
                const bool has_acc = c + 1 < width;
                if (c)   // (LK_HORNER touches neither P nor Q, and only checks its second scalar)
                    launch_lk_step(A.stream, e, acc, nullptr, nullptr, T, 0, has_acc, theta_be32, gamma_be32, A.flags());
                else
                    launch_sh_factor(A.stream, e, has_acc ? acc : nullptr, side ? D : N, q ? A.qext.as<uint32_t>() : nullptr, T,
                                     theta_be32, gamma_be32, g == 0, A.flags());
            }
        }
    }
    return grand_product_finish_dev(ctx, H, i, N, D, T, dst, out_c48, out_closing32, out_zero_den, zk, nullptr);
}

// The lookup running sum (kzg_rows_commit_lookup_sum): a set built FROM sets.  Every named row is transformed into ONE lane
// buffer and folded in as it arrives: m first (its evaluations start the numerator), the w table columns (Horner in theta from
// the last column down, the first one closes the chain and writes the fraction -m / (beta + Tb)), then the L lookups the same
// way, each adding 1 / (beta + F_l) to the running fraction P / Q.  Four vectors of T whatever L and w are (the transform's
// output, the Horner accumulator, P, Q); the transform's output is dead when the batched inversion needs its workspace.
// term = P / Q (one inversion), the additive scan turns it into S's evaluations in place, the inverse transform writes S's
// coefficients straight into the new set's buffer `dst`; one MSM commits.  The record's first two evaluation slots carry the
// closing value and the zero-denominator flag word.
// sel (kzg_rows_commit_lookup_sum_sel): each distinct selector row is transformed ONCE, in front of everything else, into a
// vector of its own in the lane's quotient workspace (sel->n vectors of T more); the lookups that name one close their Horner
// chain with LK_INPUT_SEL (numerator q_l), the others with LK_INPUT as without selectors.  Nothing else changes: the _zk mask,
// the one inversion (a zero denominator is found on every row it reads, enabled or not), the scan, the tail.
int rows_lookup_sum_dev(kzg_ctx* ctx, LaneHold& H, uint32_t i, const RowTab& inputs, const RowTab& table, const uint32_t* mult,
                        uint32_t n_lookups, uint32_t width, uint64_t T, const uint8_t* theta_be32, const uint8_t* beta_be32,
                        uint32_t* dst, uint8_t* out_c48, uint8_t* out_closing32, bool* out_zero_den, const Blind* zk,
                        const SelPlan* sel) {
    Lane& A = H.L();
    if (int rc = ensure_multi_record(ctx, A)) return rc;
    const int lg = ilog2_exact(T);
    uint32_t* tw = nullptr;
    if (int rc = ensure_twiddles(ctx, A, lg, 0, &tw, nullptr)) return rc;
    HIPCHK(ctx, A.coeffA.ensure(T * 32));
    HIPCHK(ctx, A.coeffB.ensure(T * 32));
    HIPCHK(ctx, A.bcomb.ensure(T * 32));
    HIPCHK(ctx, A.qbuf.ensure(T * 32));
    HIPCHK(ctx, A.ntt_mid.ensure(T * 48));
    HIPCHK(ctx, A.hbuf.ensure(poly_level_words(T) * 4));
    HIPCHK(ctx, A.hnext.ensure(poly_level_words(T) * 4));
    uint32_t *e = A.coeffA.as<uint32_t>(), *acc = A.coeffB.as<uint32_t>();
    uint32_t *P = A.bcomb.as<uint32_t>(), *Q = A.qbuf.as<uint32_t>(), *mid = A.ntt_mid.as<uint32_t>();
    uint8_t* rec = A.brec.as<uint8_t>();
    if (sel && sel->n) {
        HIPCHK(ctx, A.qext.ensure((size_t)sel->n * T * 32));
        Span sp(ctx, A, KZG_T_NTT);
        for (uint32_t j = 0; j < sel->n; j++)
            launch_fr_ntt(A.stream, sel->row[j], A.qext.as<uint32_t>() + (uint64_t)j * T * 8, lg, tw, nullptr, mid);
    }
    {
        Span sp(ctx, A, KZG_T_NTT);
        launch_fr_ntt(A.stream, mult, P, lg, tw, nullptr, mid);
    }
    for (uint32_t l = 0; l <= n_lookups; l++) {   // (l == 0: the table; lookup l - 1 after it)
        for (uint32_t c = width; c-- > 0;) {
            {
                Span sp(ctx, A, KZG_T_NTT);
                launch_fr_ntt(A.stream, l ? inputs.r[(l - 1) * width + c] : table.r[c], e, lg, tw, nullptr, mid);
            }
            Span sp(ctx, A, KZG_T_POLY);
            if (sel && l && !c && sel->of[l - 1] != SEL_NONE)
                launch_lk_step_sel(A.stream, e, acc, P, Q, A.qext.as<uint32_t>() + (uint64_t)sel->of[l - 1] * T * 8, T, c + 1 < width,
                                   theta_be32, beta_be32, A.flags());
            else
                launch_lk_step(A.stream, e, acc, P, Q, T, c ? 0 : (l ? 2 : 1), c + 1 < width, theta_be32, beta_be32, A.flags());
        }
    }
    {
        Span sp(ctx, A, KZG_T_POLY);
        uint32_t* zf = reinterpret_cast<uint32_t*>(rec + MR_EVAL + 32);
        // _zk: term_t = 0 / 1 on the rows >= usable, set in front of the inversion so that a zero denominator there cannot
        // poison prod Q; the unchanged scan leaves S = closing on every one of them, the tail replaces the rows behind `usable`
        if (zk) launch_blind_mask(A.stream, P, false, Q, T, zk->usable);
        launch_fr_batch_inv(A.stream, Q, e, P, P, T, A.hbuf.as<uint32_t>(), A.hnext.as<uint32_t>(), rec + MR_EVAL, zf);
        launch_lk_sum_scan(A.stream, P, T, A.hbuf.as<uint32_t>(), rec + MR_EVAL);
        if (zk) launch_blind_tail(A.stream, P, T, zk->usable, zk->tail_be32, A.flags());
    }
    const uint32_t* c;
    if (int rc = row_to_coeffs(ctx, A, P, T, 1, &c, dst)) return rc;
    uint8_t ev[64];
    if (int rc = multi_msms_finish(ctx, H, i, T, dst, 1, 0, 2, out_c48, ev, nullptr)) return rc;
    memcpy(out_closing32, ev, 32);
    uint32_t zf;
    memcpy(&zf, ev + 32, 4);
    *out_zero_den = zf != 0;
    return KZG_OK;
}

// The lookup multiplicities (kzg_rows_commit_multiplicities): a set built FROM sets, and the one row of the lookup argument
// that needs no challenge.  All w columns of a tuple must be live at once, so the workspace is 2 w vectors of T in the lane's
// quotient workspace: the w table columns in evaluation form, and the w columns of ONE lookup at a time.  The forward
// transform ends canonical (fr9_reduce) and a length-1 row is copied from a set's canonical coefficients, so the join
// (fr_join.hip) compares and hashes the words as they lie.  Build once, probe lookup by lookup into T u32 counters, turn
// the counters into m's evaluations (in the first input vector, dead by then); the inverse transform writes m's
// coefficients straight into the new set's buffer `dst`; one MSM commits.  The record's first evaluation slot carries
// `missing` (8 bytes) and the overrun flag word behind it.
// sel (kzg_rows_commit_multiplicities_sel): sel->n more vectors behind the 2 w, one per distinct selector row, transformed
// once; a lookup that names one is probed by k_join_probe_sel (only the cells whose selector is not zero), the others by the
// probe of the call without selectors.  The build, the counters, the tail and the commit are unchanged.
int rows_multiplicities_dev(kzg_ctx* ctx, LaneHold& H, uint32_t i, const RowTab& inputs, const RowTab& table, uint32_t n_lookups,
                            uint32_t width, uint64_t T, uint32_t* dst, uint8_t* out_c48, uint64_t* out_missing,
                            bool* out_overrun, const Blind* zk, const SelPlan* sel) {
    Lane& A = H.L();
    if (int rc = ensure_multi_record(ctx, A)) return rc;
    const int lg = ilog2_exact(T);
    uint32_t* tw = nullptr;
    if (int rc = ensure_twiddles(ctx, A, lg, 0, &tw, nullptr)) return rc;
    const uint64_t vw = T * 8;                 // one vector, in words
    const uint32_t cap = (uint32_t)(2 * T);    // slots: a power of two, load <= 1 / 2 (T <= 2^27: the caller)
    const uint32_t n_sel = sel ? sel->n : 0;
    HIPCHK(ctx, A.qext.ensure(((size_t)2 * width + n_sel) * T * 32));
    HIPCHK(ctx, A.qstage.ensure(((size_t)cap + T) * 4));
    HIPCHK(ctx, A.ntt_mid.ensure(T * 48));
    uint32_t *tab = A.qext.as<uint32_t>(), *in = tab + (uint64_t)width * vw, *mid = A.ntt_mid.as<uint32_t>();
    uint32_t *slots = A.qstage.as<uint32_t>(), *cnt = slots + cap;
    uint32_t* selv = in + (uint64_t)width * vw;
    uint8_t* rec = A.brec.as<uint8_t>();
    uint64_t* missing = reinterpret_cast<uint64_t*>(rec + MR_EVAL);
    uint32_t* overrun = reinterpret_cast<uint32_t*>(rec + MR_EVAL + 8);
    for (uint32_t c = 0; c < width; c++) {
        Span sp(ctx, A, KZG_T_NTT);
        launch_fr_ntt(A.stream, table.r[c], tab + c * vw, lg, tw, nullptr, mid);
    }
    for (uint32_t j = 0; j < n_sel; j++) {
        Span sp(ctx, A, KZG_T_NTT);
        launch_fr_ntt(A.stream, sel->row[j], selv + j * vw, lg, tw, nullptr, mid);
    }
    {
        Span sp(ctx, A, KZG_T_POLY);
        HIPCHK(ctx, hipMemsetAsync(slots, 0xff, (size_t)cap * 4, A.stream));
        HIPCHK(ctx, hipMemsetAsync(cnt, 0, (size_t)T * 4, A.stream));
        HIPCHK(ctx, hipMemsetAsync(rec + MR_EVAL, 0, 32, A.stream));
        // _zk: only the table rows and the cells below `usable` enter the join; the counters of the rows behind stay 0
        if (zk) launch_join_build_rows(A.stream, tab, T, zk->usable, width, slots, cap, overrun);
        else launch_join_build(A.stream, tab, T, width, slots, cap, overrun);
    }
    for (uint32_t l = 0; l < n_lookups; l++) {
        for (uint32_t c = 0; c < width; c++) {
            Span sp(ctx, A, KZG_T_NTT);
            launch_fr_ntt(A.stream, inputs.r[l * width + c], in + c * vw, lg, tw, nullptr, mid);
        }
        Span sp(ctx, A, KZG_T_POLY);
        if (sel && sel->of[l] != SEL_NONE)
            launch_join_probe_sel(A.stream, tab, in, selv + sel->of[l] * vw, T, zk ? zk->usable : T, width, slots, cap, cnt, missing,
                                  overrun);
        else if (zk) launch_join_probe_rows(A.stream, tab, in, T, zk->usable, width, slots, cap, cnt, missing, overrun);
        else launch_join_probe(A.stream, tab, in, T, width, slots, cap, cnt, missing, overrun);
    }
    {
        Span sp(ctx, A, KZG_T_POLY);
        launch_join_counts(A.stream, cnt, in, T);
        if (zk) launch_blind_tail(A.stream, in, T, zk->usable, zk->tail_be32, A.flags());
    }
    const uint32_t* c;
    if (int rc = row_to_coeffs(ctx, A, in, T, 1, &c, dst)) return rc;
    uint8_t ev[32];
    if (int rc = multi_msms_finish(ctx, H, i, T, dst, 1, 0, 1, out_c48, ev, nullptr)) return rc;
    uint32_t of;
    memcpy(out_missing, ev, 8);
    memcpy(&of, ev + 8, 4);
    *out_overrun = of != 0;
    return KZG_OK;
}

// ---- the device frame of the column builders (rows_sorted_dev, rows_derived_dev .. rows_fetch_dev): what every builder
// does around the kernels of its own.  cols_begin -- [Sources: slot_of, transform] -- the builder's kernels -- emit_column per
// output column -- stats_finish.

// The statistics of a call are u64 words in the record's evaluation slots, behind the first two (which the derived call's
// inversion uses as scratch and flag, the fetch call's join for its overrun word), and come back in the copy behind the MSM.
constexpr uint32_t CNT_OFF = 64;
constexpr uint32_t STATS_MAX = 16 * KZG_MAX_BATCH_OPEN;   // the largest user: a count and a first row for each of 16 ops
static_assert(CNT_OFF + STATS_MAX <= MR_PAIRS * 32, "the statistics of the largest builder fit the record's evaluation slots");
// what a builder's call works with: the lane's record, the forward twiddles and the transforms' scratch of T, the layout
struct Cols {
    uint64_t T, vw, n;    // the row length; one vector, in words; the rows that are read (usable, or T)
    int lg;
    uint32_t *tw, *mid, *dst;
    uint8_t* rec;
    const Blind* lay;
    uint8_t ev[CNT_OFF + STATS_MAX + 32];   // the record's evaluation slots as stats_finish read them back
};
static int cols_begin(kzg_ctx* ctx, Lane& A, uint64_t T, const Blind* lay, uint32_t* dst, Cols& F) {
    if (int rc = ensure_multi_record(ctx, A)) return rc;
    F.T = T;
    F.vw = T * 8;
    F.n = lay ? lay->usable : T;
    F.lg = ilog2_exact(T);
    F.tw = nullptr;
    if (int rc = ensure_twiddles(ctx, A, F.lg, 0, &F.tw, nullptr)) return rc;
    HIPCHK(ctx, A.ntt_mid.ensure(T * 48));
    F.mid = A.ntt_mid.as<uint32_t>();
    F.dst = dst;
    F.rec = A.brec.as<uint8_t>();
    F.lay = lay;
    return KZG_OK;
}
// The DISTINCT source rows of a call, by device pointer: several ops, both operands of one op, or two indices of a repeated
// handle, may name one row, which is transformed once.  (Capacity: what the callers of the builders let through.)
struct Sources {
    static constexpr uint32_t CAP = 3 * ALU_MAX_UNITS;
    static_assert(CAP >= POLY_MAX_ROWS && POLY_MAX_ROWS >= KZG_MAX_BATCH_OPEN, "every builder's distinct rows fit");
    const uint32_t* distinct[CAP];
    uint32_t nd = 0;
    uint32_t slot_of(const uint32_t* p) {
        uint32_t d = 0;
        while (d < nd && distinct[d] != p) d++;
        if (d == nd) distinct[nd++] = p;
        return d;
    }
};
// the forward transforms of the nd rows into the consecutive vectors at src
static void sources_transform(kzg_ctx* ctx, Lane& A, const Cols& F, const Sources& S, uint32_t* src) {
    for (uint32_t d = 0; d < S.nd; d++) {
        Span sp(ctx, A, KZG_T_NTT);
        launch_fr_ntt(A.stream, S.distinct[d], src + d * F.vw, F.lg, F.tw, nullptr, F.mid);
    }
}
// the rows a plan's factors name, as indices into `inputs`, become slots of S
static void plan_sources(ExprPlan& pl, const RowTab& inputs, Sources& S) {
    for (uint32_t u = 0; u < pl.n_terms; u++)
        for (uint32_t f = 0; f < pl.term_len[u]; f++) pl.term_row[u][f] = (uint8_t)S.slot_of(inputs.r[pl.term_row[u][f]]);
}
// output column c from the vector v: the caller's tail behind `usable` (launch_sort_tail: no closing row), then the inverse
// transform straight into the new set's buffer
static int emit_column(kzg_ctx* ctx, Lane& A, const Cols& F, uint32_t* v, uint32_t c) {
    if (F.lay) {
        Span sp(ctx, A, KZG_T_POLY);
        launch_sort_tail(A.stream, v, F.T, F.n, F.lay->tail_be32 + 32 * (size_t)c * (F.T - F.n), A.flags());
    }
    const uint32_t* cf;
    return row_to_coeffs(ctx, A, v, F.T, 1, &cf, F.dst + c * F.vw);
}
// The end of a call with `bytes` bytes of statistics: ONE MSM pass of n_out scalar sets (none for n_out = 0: the record's one
// copy and its synchronisation are all that is left).  *stats: the bytes behind CNT_OFF; F.ev: the slots in front of them
static int stats_finish(kzg_ctx* ctx, LaneHold& H, uint32_t i, Cols& F, uint32_t n_out, uint32_t bytes, uint8_t* out_c48,
                        const uint8_t** stats) {
    HIPCHK(ctx, hipGetLastError());
    const uint32_t npairs = (CNT_OFF + bytes + 31) / 32;
    if (int rc = multi_msms_finish(ctx, H, i, F.T, F.dst, n_out, 0, npairs, out_c48, F.ev, nullptr)) return rc;
    *stats = F.ev + CNT_OFF;
    return KZG_OK;
}

// ---- the unit builders' layer over Cols / Sources (rows_poseidon_dev .. rows_edwards_dev): a call is a list of units, every
// unit writes its columns side by side behind the sources and leaves a few runs of n_units u64 statistics.  A builder fills its
// kernel's table and Sources, then: units_workspace -- sources_transform -- [its constants] -- units_stats_clear --
// assign_outputs -- its launch -- units_finish.  Every call therefore has, around the steps in its builder's own table: one
// launch_fr_ntt per distinct source row named; per output row, with `usable` only, one launch_sort_tail, and one row_to_coeffs
// straight into dst; ONE multi_msms_finish pass of n_out scalar sets.

// The workspace: the S.nd source vectors at *src, the n_out output vectors at *outv, `extra` bytes behind them
static int units_workspace(kzg_ctx* ctx, Lane& A, const Cols& F, const Sources& S, uint32_t n_out, size_t extra, uint32_t** src,
                           uint32_t** outv) {
    HIPCHK(ctx, A.qext.ensure(((size_t)S.nd + n_out) * F.T * 32 + extra));
    *src = A.qext.as<uint32_t>();
    *outv = *src + S.nd * F.vw;
    return KZG_OK;
}
// the statistics in the record: `zero` runs of counts, then `none` runs of first rows (all ones: the builder's NONE)
static uint64_t* units_stats(const Cols& F) { return reinterpret_cast<uint64_t*>(F.rec + MR_EVAL + CNT_OFF); }
static int units_stats_clear(kzg_ctx* ctx, Lane& A, uint64_t* st, uint32_t n_units, uint32_t zero, uint32_t none) {
    HIPCHK(ctx, hipMemsetAsync(st, 0, 8 * (size_t)zero * n_units, A.stream));
    HIPCHK(ctx, hipMemsetAsync(st + zero * n_units, 0xff, 8 * (size_t)none * n_units, A.stream));
    return KZG_OK;
}
// tab.u[u].out for every unit that commits, in unit order.  commits(u): the number of vectors unit u commits (0: a check);
// zero_first(u): the kernel does not write every row of them
template <class Tab, class Commits, class ZeroFirst>
static int assign_outputs(kzg_ctx* ctx, Lane& A, const Cols& F, Tab& tab, uint32_t n_units, uint32_t* outv, Commits commits,
                          ZeroFirst zero_first) {
    for (uint32_t u = 0, c = 0; u < n_units; u++) {
        const uint32_t k = commits(u);
        if (!k) continue;
        tab.u[u].out = outv + c * F.vw;
        if (zero_first(u)) HIPCHK(ctx, hipMemsetAsync(outv + c * F.vw, 0, (size_t)k * F.T * 32, A.stream));
        c += k;
    }
    return KZG_OK;
}
// every output vector into the new set, ONE MSM pass, the `bytes` bytes of statistics out
static int units_finish(kzg_ctx* ctx, LaneHold& H, uint32_t i, Cols& F, uint32_t* outv, uint32_t n_out, uint32_t bytes,
                        uint8_t* out_c48, uint64_t* out_stats) {
    for (uint32_t c = 0; c < n_out; c++)
        if (int rc = emit_column(ctx, H.L(), F, outv + c * F.vw, c)) return rc;
    const uint8_t* stats;
    if (int rc = stats_finish(ctx, H, i, F, n_out, bytes, out_c48, &stats)) return rc;
    memcpy(out_stats, stats, bytes);
    return KZG_OK;
}
// a unit's own list of distinct vectors (sha256, keccak): the place of vector d in ld[0 .. n_ld), appended when it is new, so
// that a cell is loaded and counted once
static uint8_t unit_load_slot(uint8_t* ld, uint32_t& n_ld, uint8_t d) {
    uint32_t k = 0;
    while (k < n_ld && ld[k] != d) k++;
    if (k == n_ld) ld[n_ld++] = d;
    return (uint8_t)k;
}

// The sorted columns (kzg_rows_commit_sorted): a set built FROM sets, the second side of a shuffle whose first side is these
// columns.  All w columns of a row travel together, so the w columns are transformed into w vectors of T in the lane's quotient
// workspace; behind them lie the n_keys key vectors (the key columns' canonical integers: fr_sort.hip) and, in the staging
// buffer, the sort's own workspace of about 0.3 vectors (two u32 permutations, a byte per row, the per-tile counts, 8 KB of
// histograms per key column).  The front pass leaves one skip word per radix pass; their read-back (at most 2 KB, into the
// lane's pinned page) is the call's one wait before the MSM: only the passes that move something are launched after it.
// Each column is then gathered through the final permutation into one more vector (with the caller's tail behind `usable`),
// whose inverse transform writes the column's coefficients straight into the new set's buffer `dst`; ONE MSM pass of w scalar
// sets commits.  Workspace: w + n_keys + 1 vectors of T and the 0.3 above.
int rows_sorted_dev(kzg_ctx* ctx, LaneHold& H, uint32_t i, const RowTab& inputs, uint32_t width, uint32_t n_keys, uint64_t T,
                    uint32_t* dst, uint8_t* out_c48, const Blind* lay) {
    Lane& A = H.L();
    Cols F;
    if (int rc = cols_begin(ctx, A, T, lay, dst, F)) return rc;
    const uint64_t vw = F.vw, n = F.n;
    const uint32_t passes = 32 * n_keys;
    static_assert(32 * KZG_MAX_BATCH_OPEN * 4 <= 8192, "the skip words of every pass fit the lane's pinned page");
    HIPCHK(ctx, A.qext.ensure(((size_t)width + n_keys) * T * 32));
    HIPCHK(ctx, A.qstage.ensure(fr_sort_ws_words(n, n_keys) * 4));
    HIPCHK(ctx, A.coeffA.ensure(T * 32));
    uint32_t *ev = A.qext.as<uint32_t>(), *keys = ev + (uint64_t)width * vw;
    uint32_t *ws = A.qstage.as<uint32_t>(), *out = A.coeffA.as<uint32_t>();
    for (uint32_t c = 0; c < width; c++) {
        Span sp(ctx, A, KZG_T_NTT);
        launch_fr_ntt(A.stream, inputs.r[c], ev + c * vw, F.lg, F.tw, nullptr, F.mid);
    }
    {
        Span sp(ctx, A, KZG_T_POLY);
        const uint32_t* skip_dev = launch_sort_front(A.stream, ev, T, n, n_keys, keys, ws);
        HIPCHK(ctx, hipMemcpyAsync(A.bpin, skip_dev, (size_t)passes * 4, hipMemcpyDeviceToHost, A.stream));
    }
    HIPCHK(ctx, hipStreamSynchronize(A.stream));
    uint32_t skip[32 * KZG_MAX_BATCH_OPEN];
    memcpy(skip, A.bpin, (size_t)passes * 4);
    const uint32_t* perm;
    {
        Span sp(ctx, A, KZG_T_POLY);
        perm = launch_sort_passes(A.stream, keys, T, n, n_keys, skip, ws);
    }
    for (uint32_t c = 0; c < width; c++) {
        {
            Span sp(ctx, A, KZG_T_POLY);
            launch_sort_gather(A.stream, ev + c * vw, perm, out, n);
            if (lay) launch_sort_tail(A.stream, out, T, n, lay->tail_be32 + 32 * (size_t)c * (T - n), A.flags());
        }
        const uint32_t* cf;
        if (int rc = row_to_coeffs(ctx, A, out, T, 1, &cf, dst + c * vw)) return rc;
    }
    HIPCHK(ctx, hipGetLastError());
    return multi_msms_finish(ctx, H, i, T, dst, width, 0, 0, out_c48, nullptr, nullptr);
}

// The front of kzg_rows_commit_sigma and kzg_rows_check_copies: the k label columns as ONE sorted vector.  Each DISTINCT label
// row (by device pointer: two indices of a repeated handle name one row) is transformed forward once; cells [0, n) of column c
// land at cells [c n, c n + n) of `packed` (straight from the transform when n = T, through the one vector `tmp` otherwise, by
// a device copy for a repeated row), so that the flat-index order is the vector's own.  The unchanged sort then runs with
// n_keys = 1 over N = k n cells: launch_sort_front, the read-back of its 32 skip words (the call's one wait before the end),
// launch_sort_passes.  *perm: the sorted order inside ws, or null (the identity) when no pass moved anything.
static int sigma_sort_dev(kzg_ctx* ctx, Lane& A, const RowTab& labels, uint32_t k, uint64_t T, uint64_t n, const uint32_t* tw,
                          uint32_t* packed, uint32_t* tmp, uint32_t* keys, uint32_t* ws, const uint32_t** perm) {
    const int lg = ilog2_exact(T);
    const uint64_t N = (uint64_t)k * n;
    uint32_t* mid = A.ntt_mid.as<uint32_t>();
    for (uint32_t c = 0; c < k; c++) {
        uint32_t first = 0;
        while (labels.r[first] != labels.r[c]) first++;
        uint32_t* at = packed + (uint64_t)c * n * 8;
        if (first < c) {
            HIPCHK(ctx, hipMemcpyAsync(at, packed + (uint64_t)first * n * 8, n * 32, hipMemcpyDeviceToDevice, A.stream));
            continue;
        }
        Span sp(ctx, A, KZG_T_NTT);
        launch_fr_ntt(A.stream, labels.r[c], n == T ? at : tmp, lg, tw, nullptr, mid);
        if (n != T) HIPCHK(ctx, hipMemcpyAsync(at, tmp, n * 32, hipMemcpyDeviceToDevice, A.stream));
    }
    {
        Span sp(ctx, A, KZG_T_POLY);
        const uint32_t* skip_dev = launch_sort_front(A.stream, packed, N, N, 1, keys, ws);
        HIPCHK(ctx, hipMemcpyAsync(A.bpin, skip_dev, 32 * 4, hipMemcpyDeviceToHost, A.stream));
    }
    HIPCHK(ctx, hipStreamSynchronize(A.stream));
    uint32_t skip[32];
    memcpy(skip, A.bpin, sizeof(skip));
    Span sp(ctx, A, KZG_T_POLY);
    *perm = launch_sort_passes(A.stream, keys, N, N, 1, skip, ws);
    return KZG_OK;
}

// The sigma columns (kzg_rows_commit_sigma): a set built FROM sets, the permutation whose cycles are the classes of equal labels.
//   step                      launches                              per call
//   forward transforms        launch_fr_ntt                         one per distinct label row
//   sort                      launch_sort_front / _passes           n_keys = 1 over k n cells (sigma_sort_dev)
//   link + count              launch_sigma_link                     one: every cell t < n of every column
//   identity                  launch_sigma_identity                 one, with `usable` only: rows t >= n
//   inverse transform         row_to_coeffs                         one per column, straight into dst
//   commit                    multi_msms_finish                     ONE pass of k scalar sets
// The packed labels are dead once the front pass has written the keys, so the k sigma vectors take their place.  The two counts
// are u64 words behind the first two evaluation slots of the record (the layout of rows_expr_dev) and come back in the copy
// behind the MSM.  Workspace: 2 k + 1 vectors of T (sigma / packed labels, keys, one transform target; k n cells of keys and
// no target when n < T resp. n = T) and the sort's 0.3 k n elements in the staging buffer.
int rows_sigma_dev(kzg_ctx* ctx, LaneHold& H, uint32_t i, const RowTab& labels, uint32_t k, uint64_t T, uint64_t n,
                   const uint8_t* shifts_be32, const uint8_t* free_be32, uint32_t* dst, uint8_t* out_c48, uint64_t* out_stats) {
    Lane& A = H.L();
    if (int rc = ensure_multi_record(ctx, A)) return rc;
    uint32_t* tw = nullptr;
    if (int rc = ensure_twiddles(ctx, A, ilog2_exact(T), 0, &tw, nullptr)) return rc;
    const uint64_t vw = T * 8, N = (uint64_t)k * n;
    static_assert(16 <= STATS_MAX && KZG_MAX_BATCH_OPEN <= SIGMA_MAX_COLS, "the counts fit the record");
    HIPCHK(ctx, A.qext.ensure(((size_t)k * T + N + (n != T ? T : 0)) * 32));
    HIPCHK(ctx, A.qstage.ensure(fr_sort_ws_words(N, 1) * 4));
    HIPCHK(ctx, A.ntt_mid.ensure(T * 48));
    uint32_t *sig = A.qext.as<uint32_t>(), *keys = sig + (uint64_t)k * vw, *tmp = keys + N * 8, *ws = A.qstage.as<uint32_t>();
    uint8_t* rec = A.brec.as<uint8_t>();
    uint64_t* cnt = reinterpret_cast<uint64_t*>(rec + MR_EVAL + CNT_OFF);
    const uint32_t* perm = nullptr;
    if (int rc = sigma_sort_dev(ctx, A, labels, k, T, n, tw, sig, tmp, keys, ws, &perm)) return rc;
    {
        Span sp(ctx, A, KZG_T_POLY);
        HIPCHK(ctx, hipMemsetAsync(rec + MR_EVAL, 0, CNT_OFF + 16, A.stream));
        launch_sigma_link(A.stream, keys, perm, N, n, T, k, tw, shifts_be32, free_be32, sig, cnt, A.flags());
        launch_sigma_identity(A.stream, n, T, k, tw, shifts_be32, sig, A.flags());
    }
    for (uint32_t c = 0; c < k; c++) {
        const uint32_t* cf;
        if (int rc = row_to_coeffs(ctx, A, sig + c * vw, T, 1, &cf, dst + c * vw)) return rc;
    }
    HIPCHK(ctx, hipGetLastError());
    uint8_t ev[CNT_OFF + 32];
    if (int rc = multi_msms_finish(ctx, H, i, T, dst, k, 0, (CNT_OFF + 16 + 31) / 32, out_c48, ev, nullptr)) return rc;
    memcpy(out_stats, ev + CNT_OFF, 16);
    return KZG_OK;
}

// The copy check (kzg_rows_check_copies): the front of rows_sigma_dev, then ONE launch_copy_check over the k wire columns, each
// DISTINCT wire row transformed forward once.  Nothing is transformed back and no MSM runs (as a rows_expr_dev call made of
// checks alone): the record's one copy and its synchronisation end the call.  out: the violations and the smallest violating
// flat index (UINT64_MAX: none).  Workspace: 2 k n cells (packed labels, keys), the distinct wire rows and one transform
// target in vectors of T, and the sort's own.
int rows_check_copies_dev(kzg_ctx* ctx, LaneHold& H, uint32_t i, const RowTab& wires, const RowTab& labels, uint32_t k, uint64_t T,
                          uint64_t n, const uint8_t* free_be32, uint64_t* out) {
    Lane& A = H.L();
    if (int rc = ensure_multi_record(ctx, A)) return rc;
    const int lg = ilog2_exact(T);
    uint32_t* tw = nullptr;
    if (int rc = ensure_twiddles(ctx, A, lg, 0, &tw, nullptr)) return rc;
    const uint64_t vw = T * 8, N = (uint64_t)k * n;
    const uint32_t* distinct[POLY_MAX_ROWS];
    uint32_t slot[POLY_MAX_ROWS], nd = 0;
    for (uint32_t c = 0; c < k; c++) {
        uint32_t d = 0;
        while (d < nd && distinct[d] != wires.r[c]) d++;
        if (d == nd) distinct[nd++] = wires.r[c];
        slot[c] = d;
    }
    HIPCHK(ctx, A.qext.ensure((2 * N + ((size_t)nd + (n != T ? 1 : 0)) * T) * 32));
    HIPCHK(ctx, A.qstage.ensure(fr_sort_ws_words(N, 1) * 4));
    HIPCHK(ctx, A.ntt_mid.ensure(T * 48));
    uint32_t *packed = A.qext.as<uint32_t>(), *keys = packed + N * 8, *wv = keys + N * 8, *tmp = wv + (uint64_t)nd * vw;
    uint32_t *ws = A.qstage.as<uint32_t>(), *mid = A.ntt_mid.as<uint32_t>();
    uint8_t* rec = A.brec.as<uint8_t>();
    uint64_t* cnt = reinterpret_cast<uint64_t*>(rec + MR_EVAL + CNT_OFF);
    RowTab wt;
    memset(&wt, 0, sizeof(wt));
    for (uint32_t d = 0; d < nd; d++) {
        Span sp(ctx, A, KZG_T_NTT);
        launch_fr_ntt(A.stream, distinct[d], wv + d * vw, lg, tw, nullptr, mid);
    }
    for (uint32_t c = 0; c < k; c++) wt.r[c] = wv + slot[c] * vw;
    const uint32_t* perm = nullptr;
    if (int rc = sigma_sort_dev(ctx, A, labels, k, T, n, tw, packed, tmp, keys, ws, &perm)) return rc;
    {
        Span sp(ctx, A, KZG_T_POLY);
        HIPCHK(ctx, hipMemsetAsync(rec + MR_EVAL, 0, CNT_OFF + 8, A.stream));
        HIPCHK(ctx, hipMemsetAsync(cnt + 1, 0xff, 8, A.stream));   // UINT64_MAX: no violation
        launch_copy_check(A.stream, keys, perm, N, n, T, k, wt, free_be32, cnt);
    }
    HIPCHK(ctx, hipGetLastError());
    uint8_t ev[CNT_OFF + 32];
    if (int rc = multi_msms_finish(ctx, H, i, T, nullptr, 0, 0, (CNT_OFF + 16 + 31) / 32, nullptr, ev, nullptr)) return rc;
    memcpy(out, ev + CNT_OFF, 16);
    return KZG_OK;
}

// The helper columns (kzg_rows_commit_derived): a set built FROM sets, every output row a pure function of ONE source row.
// Each DISTINCT source row (by device pointer: two ops, or two indices of a repeated handle, may name one row) is transformed
// once into its own vector of the lane's quotient workspace.  All inv0 ops share ONE batched inversion: k_inv0_prepare lays
// their sources side by side with Montgomery 1 in place of every zero (and of the rows >= usable), so launch_fr_batch_inv runs
// unchanged over n_inv T elements with its one fr9_inv and nothing to flag; k_inv0_finish then writes the zeros back (and the
// bit row).  k_limbs cuts one source into its L vectors.  Every output vector takes the caller's tail behind `usable`
// (launch_sort_tail: no closing row) and is transformed straight into the new set's buffer `dst`; ONE MSM pass of n_out scalar
// sets commits.  The ops' counts are u64 words behind the first two evaluation slots of the record (which the inversion uses as
// its scratch and flag) and come back in the copy behind the MSM: the call never waits on its own.
// Workspace: distinct sources + n_inv + max(n_inv, longest op) vectors of T -- the prepared vector Q is dead behind the
// inversion, so the limb vectors and the bit row reuse it -- and T / 8 bytes of zero mask per inv0 op in the staging buffer.
int rows_derived_dev(kzg_ctx* ctx, LaneHold& H, uint32_t i, const RowTab& inputs, uint32_t n_ops, const kzg_derive_op* ops,
                     uint32_t n_out, uint64_t T, uint32_t* dst, uint8_t* out_c48, uint64_t* out_counts, const Blind* lay) {
    Lane& A = H.L();
    Cols F;
    if (int rc = cols_begin(ctx, A, T, lay, dst, F)) return rc;
    const uint64_t vw = F.vw, n = F.n;
    static_assert(8 * KZG_MAX_BATCH_OPEN <= STATS_MAX && KZG_MAX_BATCH_OPEN <= POLY_MAX_ROWS,
                  "the counts of every op (behind the inversion's scratch and flag) fit the record's evaluation slots");
    Sources S;
    uint32_t slot[POLY_MAX_ROWS], inv_op[POLY_MAX_ROWS], n_inv = 0, longest = 0;
    for (uint32_t o = 0; o < n_ops; o++) {
        slot[o] = S.slot_of(inputs.r[ops[o].row]);
        if (ops[o].kind == KZG_DERIVE_INV0) inv_op[n_inv++] = o;
        longest = std::max(longest, ops[o].kind == KZG_DERIVE_INV0 ? ops[o].count - 1 : ops[o].count);
    }
    const uint32_t mw = inv0_mask_words(T), n_scratch = std::max(n_inv, longest);
    HIPCHK(ctx, A.qext.ensure(((size_t)S.nd + n_inv + n_scratch) * T * 32));
    HIPCHK(ctx, A.qstage.ensure(((size_t)n_inv * mw + 4) * 4));
    if (n_inv) {
        HIPCHK(ctx, A.hbuf.ensure(poly_level_words(n_inv * T) * 4));
        HIPCHK(ctx, A.hnext.ensure(poly_level_words(n_inv * T) * 4));
    }
    uint32_t *src = A.qext.as<uint32_t>(), *W = src + S.nd * vw, *Q = W + n_inv * vw, *scratch = Q;
    uint32_t* mask = A.qstage.as<uint32_t>();
    uint8_t* rec = F.rec;
    uint64_t* cnt = reinterpret_cast<uint64_t*>(rec + MR_EVAL + CNT_OFF);
    sources_transform(ctx, A, F, S, src);
    HIPCHK(ctx, hipMemsetAsync(rec + MR_EVAL, 0, CNT_OFF + 8 * (size_t)n_ops, A.stream));
    if (n_inv) {
        Span sp(ctx, A, KZG_T_POLY);
        RowTab st;
        for (uint32_t j = 0; j < n_inv; j++) st.r[j] = src + slot[inv_op[j]] * vw;
        launch_inv0_prepare(A.stream, st, inv_op, n_inv, Q, mask, T, n, cnt);
        launch_fr_batch_inv(A.stream, Q, W, nullptr, W, n_inv * T, A.hbuf.as<uint32_t>(), A.hnext.as<uint32_t>(), rec + MR_EVAL,
                            reinterpret_cast<uint32_t*>(rec + MR_EVAL + 32));
    }
    uint32_t c = 0;   // the next output column
    auto emit = [&](uint32_t* v) { return emit_column(ctx, A, F, v, c++); };
    for (uint32_t o = 0, j = 0; o < n_ops; o++) {
        if (ops[o].kind == KZG_DERIVE_INV0) {
            uint32_t *inv = W + j * vw, *bit = ops[o].count == 2 ? scratch : nullptr;
            {
                Span sp(ctx, A, KZG_T_POLY);
                launch_inv0_finish(A.stream, inv, mask + (uint64_t)j * mw, T, bit);
            }
            if (int rc = emit(inv)) return rc;
            if (bit)
                if (int rc = emit(bit)) return rc;
            j++;
        } else {
            {
                Span sp(ctx, A, KZG_T_POLY);
                launch_limbs(A.stream, src + slot[o] * vw, scratch, T, n, ops[o].bits, ops[o].count, cnt + o);
            }
            for (uint32_t l = 0; l < ops[o].count; l++)
                if (int rc = emit(scratch + l * vw)) return rc;
        }
    }
    const uint8_t* st;
    if (int rc = stats_finish(ctx, H, i, F, n_out, 8 * n_ops, out_c48, &st)) return rc;
    uint32_t zf;
    memcpy(&zf, F.ev + 32, 4);
    if (zf) return fail(ctx, KZG_E_HIP, "derived: the batched inversion met a zero behind k_inv0_prepare");
    memcpy(out_counts, st, 8 * (size_t)n_ops);
    return KZG_OK;
}

// The integer ALU columns (kzg_rows_commit_int): a set built FROM sets, every output row a pure function of the canonical
// integers of ONE or TWO source rows.  Each DISTINCT source row (by device pointer: several ops, both operands of one op, or two
// indices of a repeated handle, may name one row) is transformed forward once into its own vector of the lane's quotient
// workspace.
//   step                      launches                         per call
//   forward transforms        launch_fr_ntt                    one per distinct source row named
//   every op                  launch_int (k_fr_int)            ONE, grid y = op
//   tail                      launch_sort_tail                 one per output row, with `usable` only
//   inverse transform         row_to_coeffs                    one per output row, straight into dst
//   commit                    multi_msms_finish                ONE pass of n_out scalar sets
// The outputs lie side by side behind the sources in the order of the set (op by op, row 0 then row 1), so output row c is
// vector c.  The counts and first rows are u64 words behind the first two evaluation slots of the record (the layout of the
// expression call) and come back in the copy behind the MSM: the call never waits on its own.
// Workspace: distinct sources + n_out vectors of T.
int rows_int_dev(kzg_ctx* ctx, LaneHold& H, uint32_t i, const RowTab& inputs, uint32_t n_ops, const kzg_int_op* ops, uint32_t n_out,
                 uint64_t T, uint32_t* dst, uint8_t* out_c48, uint64_t* out_counts, uint64_t* out_first, const Blind* lay) {
    Lane& A = H.L();
    Cols F;
    if (int rc = cols_begin(ctx, A, T, lay, dst, F)) return rc;
    const uint64_t vw = F.vw, n = F.n;
    static_assert(16 * KZG_MAX_BATCH_OPEN <= STATS_MAX && KZG_MAX_BATCH_OPEN <= INT_MAX_OPS,
                  "the count and the first row of every op fit the record's evaluation slots");
    Sources S;
    uint32_t sa[INT_MAX_OPS], sb[INT_MAX_OPS];
    for (uint32_t o = 0; o < n_ops; o++) {
        sa[o] = S.slot_of(inputs.r[ops[o].a]);
        sb[o] = (ops[o].flags & KZG_INT_IMM) ? UINT32_MAX : S.slot_of(inputs.r[ops[o].b]);
    }
    HIPCHK(ctx, A.qext.ensure(((size_t)S.nd + n_out) * T * 32));
    uint32_t *src = A.qext.as<uint32_t>(), *outv = src + S.nd * vw;
    uint8_t* rec = F.rec;
    uint64_t *cnt = reinterpret_cast<uint64_t*>(rec + MR_EVAL + CNT_OFF), *first = cnt + n_ops;
    sources_transform(ctx, A, F, S, src);
    HIPCHK(ctx, hipMemsetAsync(cnt, 0, 8 * (size_t)n_ops, A.stream));
    HIPCHK(ctx, hipMemsetAsync(first, 0xff, 8 * (size_t)n_ops, A.stream));   // KZG_INT_NONE
    IntTab tab;
    memset(&tab, 0, sizeof(tab));
    for (uint32_t o = 0, c = 0; o < n_ops; c += ops[o++].count) {
        IntOp& op = tab.op[o];
        op.a = src + sa[o] * vw;
        op.b = sb[o] == UINT32_MAX ? nullptr : src + sb[o] * vw;
        op.imm = ops[o].imm;
        op.out = outv + c * vw;
        op.kind = ops[o].kind;
        op.w = ops[o].width;
        op.count = ops[o].count;
    }
    {
        Span sp(ctx, A, KZG_T_POLY);
        launch_int(A.stream, tab, n_ops, T, n, cnt, first);
    }
    for (uint32_t c = 0; c < n_out; c++)
        if (int rc = emit_column(ctx, A, F, outv + c * vw, c)) return rc;
    const uint8_t* st;
    if (int rc = stats_finish(ctx, H, i, F, n_out, 16 * n_ops, out_c48, &st)) return rc;
    memcpy(out_counts, st, 8 * (size_t)n_ops);
    memcpy(out_first, st + 8 * (size_t)n_ops, 8 * (size_t)n_ops);
    return KZG_OK;
}

// The ALU column with an op-code column (kzg_rows_commit_alu), in the builders' frame.  Each DISTINCT source row (by device
// pointer: the op-code column and both operands of one unit, or rows of several units, may be one row) is transformed forward
// once; column b of a unit is not transformed when every entry of the program has an immediate.
//   step                      launches                         per call
//   forward transforms        launch_fr_ntt                    one per distinct source row named
//   every unit                launch_alu (k_fr_alu)            ONE, grid y = unit
//   tail                      launch_sort_tail                 one per output row, with `usable` only
//   inverse transform         row_to_coeffs                    one per output row, straight into dst
//   commit                    multi_msms_finish                ONE pass of n_out scalar sets
// The outputs lie side by side behind the sources, unit by unit, row 0 then row 1.  The four u64 statistics of every unit lie
// in the record's evaluation slots where rows_int_dev keeps its two (at most 8 units x 32 B = the 256 B of 16 ops x 16 B) and
// come back in the copy behind the MSM.  Workspace: distinct sources + n_out vectors of T.
int rows_alu_dev(kzg_ctx* ctx, LaneHold& H, uint32_t i, const RowTab& inputs, uint32_t n_entries, const kzg_alu_entry* program,
                 uint32_t n_units, const kzg_alu_unit* units, uint32_t n_out, uint64_t T, uint32_t* dst, uint8_t* out_c48,
                 uint64_t* out_stats, const Blind* lay) {
    Lane& A = H.L();
    Cols F;
    if (int rc = cols_begin(ctx, A, T, lay, dst, F)) return rc;
    const uint64_t vw = F.vw, n = F.n;
    static_assert(32 * KZG_ALU_MAX_UNITS <= STATS_MAX && KZG_ALU_MAX_UNITS == ALU_MAX_UNITS && KZG_ALU_MAX_PROGRAM == ALU_MAX_PROG,
                  "the four statistics of every unit (counts, unknown, first, first unknown) fit the record's evaluation slots");
    bool needs_b = false;
    for (uint32_t e = 0; e < n_entries; e++) needs_b |= program[e].kind != KZG_ALU_IDLE && !(program[e].flags & KZG_ALU_IMM);
    static_assert(3 * ALU_MAX_UNITS <= Sources::CAP, "the op-code column and both operands of every unit");
    Sources S;
    uint32_t so[ALU_MAX_UNITS], sa[ALU_MAX_UNITS], sb[ALU_MAX_UNITS];
    for (uint32_t u = 0; u < n_units; u++) {
        so[u] = S.slot_of(inputs.r[units[u].op_row]);
        sa[u] = S.slot_of(inputs.r[units[u].a]);
        sb[u] = needs_b ? S.slot_of(inputs.r[units[u].b]) : UINT32_MAX;
    }
    HIPCHK(ctx, A.qext.ensure(((size_t)S.nd + n_out) * T * 32));
    uint32_t *src = A.qext.as<uint32_t>(), *outv = src + S.nd * vw;
    uint8_t* rec = F.rec;
    uint64_t* st = reinterpret_cast<uint64_t*>(rec + MR_EVAL + CNT_OFF);
    sources_transform(ctx, A, F, S, src);
    HIPCHK(ctx, hipMemsetAsync(st, 0, 16 * (size_t)n_units, A.stream));
    HIPCHK(ctx, hipMemsetAsync(st + 2 * n_units, 0xff, 16 * (size_t)n_units, A.stream));   // KZG_ALU_NONE
    AluTab tab;
    memset(&tab, 0, sizeof(tab));
    for (uint32_t e = 0; e < n_entries; e++) {
        tab.prog[e].imm = program[e].imm;
        tab.prog[e].kind = program[e].kind;
        tab.prog[e].w_imm = program[e].width | ((program[e].flags & KZG_ALU_IMM) ? 0x100u : 0u);
    }
    for (uint32_t u = 0, c = 0; u < n_units; c += units[u++].count) {
        AluUnit& un = tab.unit[u];
        un.op = src + so[u] * vw;
        un.a = src + sa[u] * vw;
        un.b = sb[u] == UINT32_MAX ? nullptr : src + sb[u] * vw;
        un.out = outv + c * vw;
        un.count = units[u].count;
    }
    {
        Span sp(ctx, A, KZG_T_POLY);
        launch_alu(A.stream, tab, n_entries, n_units, T, n, st);
    }
    for (uint32_t c = 0; c < n_out; c++)
        if (int rc = emit_column(ctx, A, F, outv + c * vw, c)) return rc;
    const uint8_t* stats;
    if (int rc = stats_finish(ctx, H, i, F, n_out, 32 * n_units, out_c48, &stats)) return rc;
    memcpy(out_stats, stats, 32 * (size_t)n_units);
    return KZG_OK;
}

// The multi-limb integer columns (kzg_rows_commit_wide), in the builders' frame.  Each DISTINCT source row (by device
// pointer) among the limb rows that some operand names is transformed forward once; an operand is the list of its limbs' slots.
//   step                      launches                         per call
//   forward transforms        launch_fr_ntt                    one per distinct source row named
//   every op                  launch_wide (k_fr_wide<N>)       ONE, grid y = op
//   tail                      launch_sort_tail                 one per output row, with `usable` only
//   inverse transform         row_to_coeffs                    one per output row, straight into dst
//   commit                    multi_msms_finish                ONE pass of n_out scalar sets
// The four u64 statistics of every op lie in the record's evaluation slots where rows_alu_dev keeps its four and come back in
// the copy behind the MSM.  Workspace: distinct sources + n_out vectors of T.
static void wide_words(uint32_t w[16], const uint8_t be64[64]) {
    for (int i = 0; i < 16; i++)
        w[i] = ((uint32_t)be64[60 - 4 * i] << 24) | ((uint32_t)be64[61 - 4 * i] << 16) | ((uint32_t)be64[62 - 4 * i] << 8) |
               be64[63 - 4 * i];
}
int rows_wide_dev(kzg_ctx* ctx, LaneHold& H, uint32_t i, const RowTab& inputs, uint32_t n_ops, const kzg_wide_op* ops,
                  uint32_t n_out, uint64_t T, uint32_t* dst, uint8_t* out_c48, uint64_t* out_stats, const Blind* lay) {
    Lane& A = H.L();
    Cols F;
    if (int rc = cols_begin(ctx, A, T, lay, dst, F)) return rc;
    const uint64_t vw = F.vw, n = F.n;
    static_assert(32 * KZG_WIDE_MAX_OPS <= STATS_MAX && KZG_WIDE_MAX_OPS == WIDE_MAX_OPS && KZG_WIDE_MAX_LIMBS == WIDE_MAX_LIMBS,
                  "the four statistics of every op (counts, qover, first, first qover) fit the record's evaluation slots");
    Sources S;
    WideTab tab;
    memset(&tab, 0, sizeof(tab));
    for (uint32_t o = 0; o < n_ops; o++) {
        const kzg_wide_op& in = ops[o];
        WideOp& op = tab.op[o];
        const uint32_t first[5] = {in.a, in.b, in.c, in.q, in.r};
        for (int w = 0; w < 5; w++)
            for (uint32_t l = 0; l < in.limbs && first[w] != KZG_WIDE_ABSENT; l++)
                op.slot[w][l] = (uint8_t)S.slot_of(inputs.r[first[w] + l]);
        op.kind = in.kind;
        op.bits = in.bits;
        op.limbs = in.limbs;
        op.count = in.count;
        op.flags = in.flags & KZG_WIDE_NEG_C;
        if (in.b != KZG_WIDE_ABSENT) {
            op.flags |= WIDE_F_ROW_B;
            if (memcmp(op.slot[WIDE_A], op.slot[WIDE_B], in.limbs) == 0) op.flags |= WIDE_F_B_IS_A;
        }
        if (in.c != KZG_WIDE_ABSENT) op.flags |= WIDE_F_ROW_C;
        wide_words(op.imm, in.imm_be64);
        if (in.b == KZG_WIDE_ABSENT && !(in.flags & KZG_WIDE_IMM_B)) op.imm[0] = 1;   // no b: a times 1
        wide_words(op.m, in.m_be64);
    }
    HIPCHK(ctx, A.qext.ensure(((size_t)S.nd + n_out) * T * 32));
    uint32_t *src = A.qext.as<uint32_t>(), *outv = src + S.nd * vw;
    uint8_t* rec = F.rec;
    uint64_t* st = reinterpret_cast<uint64_t*>(rec + MR_EVAL + CNT_OFF);
    sources_transform(ctx, A, F, S, src);
    HIPCHK(ctx, hipMemsetAsync(st, 0, 16 * (size_t)n_ops, A.stream));
    HIPCHK(ctx, hipMemsetAsync(st + 2 * n_ops, 0xff, 16 * (size_t)n_ops, A.stream));   // KZG_INT_NONE
    tab.src = src;
    for (uint32_t o = 0, c = 0; o < n_ops; c += ops[o++].count) tab.op[o].out = outv + c * vw;
    {
        Span sp(ctx, A, KZG_T_POLY);
        launch_wide(A.stream, tab, n_ops, T, n, st);
    }
    for (uint32_t c = 0; c < n_out; c++)
        if (int rc = emit_column(ctx, A, F, outv + c * vw, c)) return rc;
    const uint8_t* stats;
    if (int rc = stats_finish(ctx, H, i, F, n_out, 32 * n_ops, out_c48, &stats)) return rc;
    memcpy(out_stats, stats, 32 * (size_t)n_ops);
    return KZG_OK;
}

// The Poseidon permutation columns (kzg_rows_commit_poseidon), in the builders' frame, with checks as rows_expr_dev has them.
// Each DISTINCT source row (by device pointer) that some unit reads or expects is transformed forward once.
//   step                      launches                         per call
//   constants                 one host-to-device copy          rc, M and the immediates as words, behind the vectors
//   zero the trace columns    hipMemsetAsync                   one per ROUNDS unit
//   every unit                launch_poseidon (k_fr_poseidon<t>) ONE, grid y = unit
// The mismatch count and the first mismatching row of every unit are u64 words behind the first two evaluation slots of the
// record (the layout of rows_expr_dev) and come back in the copy behind the MSM.  With n_out = 0 (checks alone) nothing is
// transformed back and no MSM runs.  Workspace: distinct sources + n_out vectors of T, and the constants.
static void poseidon_words(uint32_t w[8], const uint8_t* be32) {
    for (int i = 0; i < 8; i++)
        w[i] = ((uint32_t)be32[28 - 4 * i] << 24) | ((uint32_t)be32[29 - 4 * i] << 16) | ((uint32_t)be32[30 - 4 * i] << 8) |
               be32[31 - 4 * i];
}
// rc, M and every unit's t immediates as words, in the order of poseidon_cst_words (both Poseidon builders)
template <class Unit>
static std::vector<uint32_t> poseidon_constants(const kzg_poseidon_params* params, uint32_t n_units, const Unit* units) {
    const uint32_t t = params->t, R = params->full + params->partial;
    std::vector<uint32_t> cst(poseidon_cst_words(t, R, n_units), 0);
    for (uint32_t k = 0; k < t * R; k++) poseidon_words(&cst[8 * k], params->rc_be32 + 32 * (size_t)k);
    for (uint32_t k = 0; k < t * t; k++) poseidon_words(&cst[8 * (t * R + k)], params->mds_be32 + 32 * (size_t)k);
    for (uint32_t u = 0; u < n_units; u++)
        for (uint32_t j = 0; j < t; j++) poseidon_words(&cst[8 * (t * R + t * t + u * t + j)], units[u].imm_be32[j]);
    return cst;
}
// the constants of kzg_rows_commit_poseidon2 in the order of poseidon2_cst_words: rc_full, rc_partial, diag, every unit's immediates
static std::vector<uint32_t> poseidon2_constants(const kzg_poseidon2_params* params, uint32_t n_units,
                                                 const kzg_poseidon_unit* units) {
    const uint32_t t = params->t, nf = t * params->full, np = params->partial;
    std::vector<uint32_t> cst(poseidon2_cst_words(t, params->full, np, n_units), 0);
    for (uint32_t k = 0; k < nf; k++) poseidon_words(&cst[8 * k], params->rc_full_be32 + 32 * (size_t)k);
    for (uint32_t k = 0; k < np; k++) poseidon_words(&cst[8 * (nf + k)], params->rc_partial_be32 + 32 * (size_t)k);
    for (uint32_t k = 0; k < t; k++) poseidon_words(&cst[8 * (nf + np + k)], params->diag_be32 + 32 * (size_t)k);
    for (uint32_t u = 0; u < n_units; u++)
        for (uint32_t j = 0; j < t; j++) poseidon_words(&cst[8 * (nf + np + t + u * t + j)], units[u].imm_be32[j]);
    return cst;
}
// The body of rows_poseidon_dev and rows_poseidon2_dev: the table of the units, the steps above, `launch` the builder's kernel;
// cst: its constants as words (they live until the MSM pass has waited)
static int poseidon_units_dev(kzg_ctx* ctx, LaneHold& H, uint32_t i, const RowTab& inputs, uint32_t t, uint32_t full,
                              uint32_t partial, const std::vector<uint32_t>& cst,
                              void (*launch)(hipStream_t, const PosTab&, uint64_t, uint64_t, uint64_t*), uint32_t n_units,
                              const kzg_poseidon_unit* units, uint32_t n_out, uint64_t T, uint32_t* dst, uint8_t* out_c48,
                              uint64_t* out_stats, const Blind* lay) {
    Lane& A = H.L();
    Cols F;
    if (int rc = cols_begin(ctx, A, T, lay, dst, F)) return rc;
    const uint64_t vw = F.vw, n = F.n;
    static_assert(16 * KZG_POSEIDON_MAX_UNITS <= STATS_MAX && KZG_POSEIDON_MAX_UNITS == POS_MAX_UNITS &&
                      KZG_POSEIDON_MAX_T == POS_MAX_T && KZG_POSEIDON_MAX_FULL + KZG_POSEIDON_MAX_PARTIAL == POS_MAX_ROUNDS &&
                      KZG_POSEIDON_ROW == POS_ROW && KZG_POSEIDON_ROUNDS == POS_ROUNDS,
                  "the two statistics of every unit (mismatches, then the first rows) fit the record's evaluation slots; the "
                  "header's caps are the kernel's");
    Sources S;
    PosTab tab;
    memset(&tab, 0, sizeof(tab));
    tab.t = t;
    tab.full = full;
    tab.partial = partial;
    tab.n_units = n_units;
    const uint32_t cw = (uint32_t)cst.size();
    for (uint32_t u = 0; u < n_units; u++) {
        const kzg_poseidon_unit& in = units[u];
        PosUnit& U = tab.u[u];
        const bool check = in.flags & KZG_POSEIDON_CHECK;
        U.mode = in.mode;
        U.period = in.period;
        memset(U.col, POS_NO_COL, sizeof(U.col));
        for (uint32_t j = 0; j < t; j++)
            U.slot[j] = in.in[j] == KZG_POSEIDON_IMM ? (uint8_t)POS_IMM : (uint8_t)S.slot_of(inputs.r[in.in[j]]);
        for (uint32_t c = 0; c < in.n_out; c++) {
            U.col[in.out[c]] = (uint8_t)c;
            if (check) U.exp[c] = (uint8_t)S.slot_of(inputs.r[in.expect[c]]);
        }
    }
    uint32_t *src, *outv;
    if (int rc = units_workspace(ctx, A, F, S, n_out, (size_t)cw * 4, &src, &outv)) return rc;
    uint32_t* cdev = outv + n_out * vw;
    uint64_t* st = units_stats(F);
    sources_transform(ctx, A, F, S, src);
    HIPCHK(ctx, hipMemcpyAsync(cdev, cst.data(), (size_t)cw * 4, hipMemcpyHostToDevice, A.stream));
    if (int rc = units_stats_clear(ctx, A, st, n_units, 1, 1)) return rc;
    tab.src = src;
    tab.cst = cdev;
    if (int rc = assign_outputs(
            ctx, A, F, tab, n_units, outv, [&](uint32_t u) { return units[u].flags & KZG_POSEIDON_CHECK ? 0u : units[u].n_out; },
            [&](uint32_t u) { return units[u].mode == KZG_POSEIDON_ROUNDS; }))   // (a ROUNDS unit commits n_out = t columns)
        return rc;
    {
        Span sp(ctx, A, KZG_T_POLY);
        launch(A.stream, tab, T, n, st);
    }
    return units_finish(ctx, H, i, F, outv, n_out, 16 * n_units, out_c48, out_stats);
}
int rows_poseidon_dev(kzg_ctx* ctx, LaneHold& H, uint32_t i, const RowTab& inputs, const kzg_poseidon_params* params,
                      uint32_t n_units, const kzg_poseidon_unit* units, uint32_t n_out, uint64_t T, uint32_t* dst,
                      uint8_t* out_c48, uint64_t* out_stats, const Blind* lay) {
    return poseidon_units_dev(ctx, H, i, inputs, params->t, params->full, params->partial,
                              poseidon_constants(params, n_units, units), launch_poseidon, n_units, units, n_out, T, dst, out_c48,
                              out_stats, lay);
}
// The Poseidon2 permutation columns (kzg_rows_commit_poseidon2): the frame, the steps and the statistics of rows_poseidon_dev
// with launch_poseidon2 (k_fr_poseidon2<t>) and its constants: t R_F + R_P + t scalars and the immediates
int rows_poseidon2_dev(kzg_ctx* ctx, LaneHold& H, uint32_t i, const RowTab& inputs, const kzg_poseidon2_params* params,
                       uint32_t n_units, const kzg_poseidon_unit* units, uint32_t n_out, uint64_t T, uint32_t* dst,
                       uint8_t* out_c48, uint64_t* out_stats, const Blind* lay) {
    static_assert(16 * KZG_POSEIDON2_MAX_UNITS <= STATS_MAX && KZG_POSEIDON2_MAX_UNITS == POS_MAX_UNITS &&
                      KZG_POSEIDON2_MAX_FULL + KZG_POSEIDON2_MAX_PARTIAL == POS_MAX_ROUNDS && (KZG_POSEIDON2_WIDTHS >> (POS_MAX_T + 1)) == 0,
                  "the two statistics of every unit fit the record's evaluation slots; the header's caps are the kernel's");
    return poseidon_units_dev(ctx, H, i, inputs, params->t, params->full, params->partial,
                              poseidon2_constants(params, n_units, units), launch_poseidon2, n_units, units, n_out, T, dst,
                              out_c48, out_stats, lay);
}

// The Poseidon sponge and Merkle-path chains (kzg_rows_commit_poseidon_chain), in the builders' frame, with checks as
// rows_poseidon_dev has them.  Each DISTINCT source row (by device pointer) that some unit reads is transformed forward once.
//   step                      launches                         per call
//   constants                 one host-to-device copy          rc, M and the immediates as words, behind the vectors
//   zero the columns          hipMemsetAsync                   one per committing unit
//   every unit                launch_poseidon_chain (k_fr_poseidon_chain<t>) ONE, grid y = unit
// The five statistics of every unit are u64 words behind the first two evaluation slots of the record and come back in the copy
// behind the MSM.  With n_out = 0 (checks alone) nothing is transformed back and no MSM runs.  Workspace: distinct sources + n_out
// vectors of T, and the constants.
int rows_poseidon_chain_dev(kzg_ctx* ctx, LaneHold& H, uint32_t i, const RowTab& inputs, const kzg_poseidon_params* params,
                            uint32_t n_units, const kzg_poseidon_chain_unit* units, uint32_t n_out, uint64_t T, uint32_t* dst,
                            uint8_t* out_c48, uint64_t* out_stats, const Blind* lay) {
    Lane& A = H.L();
    Cols F;
    if (int rc = cols_begin(ctx, A, T, lay, dst, F)) return rc;
    const uint64_t vw = F.vw, n = F.n;
    static_assert(40 * KZG_POSEIDON_CHAIN_MAX_UNITS <= STATS_MAX && KZG_POSEIDON_CHAIN_MAX_UNITS == PCH_MAX_UNITS &&
                      KZG_POSEIDON_CHAIN_SPONGE == PCH_SPONGE && KZG_POSEIDON_CHAIN_PATH == PCH_PATH &&
                      KZG_POSEIDON_CHAIN_TRACE == PCH_TRACE && KZG_POSEIDON_CHAIN_FLAT == PCH_FLAT &&
                      KZG_POSEIDON_CHAIN_COL_OUT == POS_MAX_T && KZG_MAX_BATCH_OPEN <= Sources::CAP,
                  "the five statistics of every unit fit the record's evaluation slots; the header's values are the kernel's");
    const uint32_t t = params->t, R = params->full + params->partial;
    Sources S;
    PchTab tab;
    memset(&tab, 0, sizeof(tab));
    tab.t = t;
    tab.full = params->full;
    tab.partial = params->partial;
    tab.n_units = n_units;
    const std::vector<uint32_t> cst = poseidon_constants(params, n_units, units);   // (lives until the MSM pass has waited)
    const uint32_t cw = (uint32_t)cst.size();
    auto slot = [&](uint32_t row) { return row == KZG_POSEIDON_CHAIN_ABSENT ? (uint8_t)PCH_NONE : (uint8_t)S.slot_of(inputs.r[row]); };
    for (uint32_t u = 0; u < n_units; u++) {
        const kzg_poseidon_chain_unit& in = units[u];
        PchUnit& U = tab.u[u];
        U.mode = in.mode;
        U.layout = in.layout;
        U.period = in.period;
        memset(U.col, PCH_NONE, sizeof(U.col));
        memset(U.slot, PCH_NONE, sizeof(U.slot));
        for (uint32_t j = 0; j < t; j++) U.slot[j] = slot(in.in[j]);   // (KZG_POSEIDON_IMM is KZG_POSEIDON_CHAIN_ABSENT's value)
        if (in.layout == KZG_POSEIDON_CHAIN_FLAT)
            for (uint32_t c = 0; c < in.n_out; c++) U.col[in.out[c]] = (uint8_t)c;
        U.start = slot(in.start);
        U.pos = slot(in.pos);
        U.exp = slot(in.expect);
        U.digest = in.digest == KZG_POSEIDON_CHAIN_ABSENT ? (uint8_t)PCH_NONE : (uint8_t)in.digest;
    }
    uint32_t *src, *outv;
    if (int rc = units_workspace(ctx, A, F, S, n_out, (size_t)cw * 4, &src, &outv)) return rc;
    uint32_t* cdev = outv + n_out * vw;
    uint64_t* st = units_stats(F);
    sources_transform(ctx, A, F, S, src);
    HIPCHK(ctx, hipMemcpyAsync(cdev, cst.data(), (size_t)cw * 4, hipMemcpyHostToDevice, A.stream));
    if (int rc = units_stats_clear(ctx, A, st, n_units, 3, 2)) return rc;
    tab.src = src;
    tab.cst = cdev;
    if (int rc = assign_outputs(
            ctx, A, F, tab, n_units, outv, [&](uint32_t u) { return units[u].n_out; }, [](uint32_t) { return true; }))   // (0: a check)
        return rc;
    {
        Span sp(ctx, A, KZG_T_POLY);
        launch_poseidon_chain(A.stream, tab, T, n, st);
    }
    return units_finish(ctx, H, i, F, outv, n_out, 40 * n_units, out_c48, out_stats);
}

// The SHA-256 compression columns (kzg_rows_commit_sha256), in the builders' frame, with checks as rows_poseidon_dev has them.
// Each DISTINCT source row (by device pointer) that some unit reads or expects is transformed forward once.
//   step                      launches                         per call
//   zero the trace columns    hipMemsetAsync                   one per ROUNDS unit
//   every unit                launch_sha256 (k_fr_sha256)      ONE, grid y = unit
// The five statistics of every unit are u64 words behind the first two evaluation slots of the record and come back in the copy
// behind the MSM.  With n_out = 0 (checks alone) nothing is transformed back and no MSM runs.  The standard initial value is
// written into the unit's immediates here.  Workspace: distinct sources + n_out vectors of T.
int rows_sha256_dev(kzg_ctx* ctx, LaneHold& H, uint32_t i, const RowTab& inputs, uint32_t n_units, const kzg_sha256_unit* units,
                    uint32_t n_out, uint64_t T, uint32_t* dst, uint8_t* out_c48, uint64_t* out_stats, const Blind* lay) {
    Lane& A = H.L();
    Cols F;
    if (int rc = cols_begin(ctx, A, T, lay, dst, F)) return rc;
    const uint64_t vw = F.vw, n = F.n;
    static_assert(40 * KZG_SHA256_MAX_UNITS <= STATS_MAX && KZG_SHA256_MAX_UNITS == SHA_MAX_UNITS && KZG_SHA256_ROW == SHA_ROW &&
                      KZG_SHA256_ROUNDS == SHA_ROUNDS && KZG_SHA256_MIN_PERIOD == SHA_MIN_PERIOD && KZG_SHA256_N_COLS == SHA_N_COLS &&
                      KZG_SHA256_COL_W == SHA_COL_W && KZG_SHA256_COL_CE == SHA_COL_CE && KZG_SHA256_COL_CH == SHA_COL_CH,
                  "the five statistics of every unit fit the record's evaluation slots; the header's caps and column ids are the "
                  "kernel's");
    static const uint32_t std_iv[8] = {0x6a09e667u, 0xbb67ae85u, 0x3c6ef372u, 0xa54ff53au, 0x510e527fu, 0x9b05688cu, 0x1f83d9abu, 0x5be0cd19u};
    Sources S;
    ShaTab tab;
    memset(&tab, 0, sizeof(tab));
    tab.n_units = n_units;
    for (uint32_t u = 0; u < n_units; u++) {
        const kzg_sha256_unit& in = units[u];
        ShaUnit& U = tab.u[u];
        const bool rounds = in.mode == KZG_SHA256_ROUNDS;
        U.mode = in.mode;
        U.period = in.period;
        U.n_out = in.n_out;
        for (uint32_t j = 0; j < 8; j++) U.imm[j] = (in.flags & KZG_SHA256_STD_IV) ? std_iv[j] : in.state_imm[j];
        for (uint32_t c = 0; c < in.n_out; c++) {
            U.col[c] = (uint8_t)in.out[c];
            if (in.flags & KZG_SHA256_CHECK) U.exp[c] = (uint8_t)S.slot_of(inputs.r[in.expect[c]]);
        }
        memset(U.slot, SHA_IMM, sizeof(U.slot));
        if (rounds) {
            U.ld[0] = (uint8_t)S.slot_of(inputs.r[in.msg[0]]);
            U.ld[1] = in.start == KZG_SHA256_ABSENT ? (uint8_t)SHA_IMM : (uint8_t)S.slot_of(inputs.r[in.start]);
            continue;
        }
        for (uint32_t j = 0; j < 24; j++) {   // the unit's own list of distinct vectors: a cell is loaded and counted once
            const uint32_t row = j < 8 ? in.state[j] : in.msg[j - 8];
            if (j >= 8) U.imm[j] = in.msg_imm[j - 8];
            if (row == KZG_SHA256_IMM) continue;
            U.slot[j] = unit_load_slot(U.ld, U.n_ld, (uint8_t)S.slot_of(inputs.r[row]));
        }
    }
    uint32_t *src, *outv;   // (+ 32: a call of immediates alone and checks has no vector)
    if (int rc = units_workspace(ctx, A, F, S, n_out, 32, &src, &outv)) return rc;
    uint64_t* st = units_stats(F);
    sources_transform(ctx, A, F, S, src);
    if (int rc = units_stats_clear(ctx, A, st, n_units, 3, 2)) return rc;
    tab.src = src;
    if (int rc = assign_outputs(
            ctx, A, F, tab, n_units, outv, [&](uint32_t u) { return units[u].flags & KZG_SHA256_CHECK ? 0u : units[u].n_out; },
            [&](uint32_t u) { return units[u].mode == KZG_SHA256_ROUNDS; }))
        return rc;
    {
        Span sp(ctx, A, KZG_T_POLY);
        launch_sha256(A.stream, tab, T, n, st);
    }
    return units_finish(ctx, H, i, F, outv, n_out, 40 * n_units, out_c48, out_stats);
}

// The Keccak-f[1600] permutation columns (kzg_rows_commit_keccak), in the builders' frame, step for step as rows_sha256_dev:
//   step                      launches                         per call
//   zero the trace columns    hipMemsetAsync                   one per ROUNDS unit
//   every unit                launch_keccak (k_fr_keccak)      ONE, grid y = unit
// The five statistics of every unit are u64 words behind the first two evaluation slots of the record and come back in the copy
// behind the MSM.  With n_out = 0 (checks alone) nothing is transformed back and no MSM runs.  A cell that several absorbed
// lanes of a ROUNDS unit read (a repeated message row, the start column among the message rows) is marked here so that one
// reader counts it.  Workspace: distinct sources + n_out vectors of T.
int rows_keccak_dev(kzg_ctx* ctx, LaneHold& H, uint32_t i, const RowTab& inputs, uint32_t n_units, const kzg_keccak_unit* units,
                    uint32_t n_out, uint64_t T, uint32_t* dst, uint8_t* out_c48, uint64_t* out_stats, const Blind* lay) {
    Lane& A = H.L();
    Cols F;
    if (int rc = cols_begin(ctx, A, T, lay, dst, F)) return rc;
    const uint64_t vw = F.vw, n = F.n;
    static_assert(40 * KZG_KECCAK_MAX_UNITS <= STATS_MAX && KZG_KECCAK_MAX_UNITS == KEC_MAX_UNITS && KZG_KECCAK_ROW == KEC_ROW &&
                      KZG_KECCAK_ROUNDS == KEC_ROUNDS && KZG_KECCAK_MIN_PERIOD == KEC_MIN_PERIOD && KZG_KECCAK_N_COLS == KEC_N_COLS &&
                      KZG_KECCAK_MAX_OUT == KEC_MAX_OUT && KZG_KECCAK_COL_A == KEC_COL_A && KZG_KECCAK_COL_P == KEC_COL_P &&
                      KZG_KECCAK_COL_D == KEC_COL_D && KZG_KECCAK_COL_T == KEC_COL_T && KZG_KECCAK_COL_B == KEC_COL_B,
                  "the five statistics of every unit fit the record's evaluation slots; the header's caps and column ids are the "
                  "kernel's");
    Sources S;
    KecTab tab;
    memset(&tab, 0, sizeof(tab));
    tab.n_units = n_units;
    for (uint32_t u = 0; u < n_units; u++) {
        const kzg_keccak_unit& in = units[u];
        KecUnit& U = tab.u[u];
        const bool rounds = in.mode == KZG_KECCAK_ROUNDS;
        U.mode = in.mode;
        U.period = in.period;
        U.rate = in.rate;
        U.n_out = in.n_out;
        for (uint32_t c = 0; c < in.n_out; c++) {
            U.col[c] = (uint8_t)in.out[c];
            if (in.flags & KZG_KECCAK_CHECK) U.exp[c] = (uint8_t)S.slot_of(inputs.r[in.expect[c]]);
        }
        memset(U.slot, KEC_IMM, sizeof(U.slot));
        if (rounds) {
            for (uint32_t x = 0; x < 5; x++) U.ld[x] = (uint8_t)S.slot_of(inputs.r[in.in[x]]);
            U.ld[5] = in.start == KZG_KECCAK_ABSENT ? (uint8_t)KEC_IMM : (uint8_t)S.slot_of(inputs.r[in.start]);
            for (uint32_t l = 0; l < in.rate; l++) {
                const uint32_t x = l % 5;
                bool counted = l < 5 && U.ld[x] == U.ld[5];
                for (uint32_t k = 0; k < x; k++) counted |= U.ld[k] == U.ld[x];
                U.nocount |= (uint32_t)counted << l;
            }
            continue;
        }
        for (uint32_t j = 0; j < 25; j++) {   // the unit's own list of distinct vectors: a cell is loaded and counted once
            U.imm[j] = in.imm[j];
            if (in.in[j] == KZG_KECCAK_IMM) continue;
            U.slot[j] = unit_load_slot(U.ld, U.n_ld, (uint8_t)S.slot_of(inputs.r[in.in[j]]));
        }
    }
    uint32_t *src, *outv;   // (+ 32: a call of immediates alone and checks has no vector)
    if (int rc = units_workspace(ctx, A, F, S, n_out, 32, &src, &outv)) return rc;
    uint64_t* st = units_stats(F);
    sources_transform(ctx, A, F, S, src);
    if (int rc = units_stats_clear(ctx, A, st, n_units, 3, 2)) return rc;
    tab.src = src;
    if (int rc = assign_outputs(
            ctx, A, F, tab, n_units, outv, [&](uint32_t u) { return units[u].flags & KZG_KECCAK_CHECK ? 0u : units[u].n_out; },
            [&](uint32_t u) { return units[u].mode == KZG_KECCAK_ROUNDS; }))
        return rc;
    {
        Span sp(ctx, A, KZG_T_POLY);
        launch_keccak(A.stream, tab, T, n, st);
    }
    return units_finish(ctx, H, i, F, outv, n_out, 40 * n_units, out_c48, out_stats);
}

// The non-native elliptic-curve columns (kzg_rows_commit_ec), in the builders' frame, step for step as rows_keccak_dev:
//   step                      launches                         per call
//   every unit                launch_ec (k_fr_ec)              ONE, grid y = unit
// The seven statistics of every unit are u64 words behind the first two evaluation slots of the record and come back in the
// copy behind the MSM.  With n_out = 0 (checks alone) nothing is transformed back and no MSM runs.  The curve's two derived
// constants are computed here, on the host, once per call: -p^-1 mod 2^32 by Newton's iteration and 2^512 mod p by 512
// doublings.  Every row t < n of a committed column is written by the kernel (a CHAIN unit's rows by the lane of their
// segment), so nothing is zeroed first.  Workspace: distinct sources + n_out vectors of T.
int rows_ec_dev(kzg_ctx* ctx, LaneHold& H, uint32_t i, const RowTab& inputs, const kzg_ec_curve* curve, uint32_t n_units,
                const kzg_ec_unit* units, uint32_t n_out, uint64_t T, uint32_t* dst, uint8_t* out_c48, uint64_t* out_stats,
                const Blind* lay) {
    Lane& A = H.L();
    Cols F;
    if (int rc = cols_begin(ctx, A, T, lay, dst, F)) return rc;
    const uint64_t vw = F.vw, n = F.n;
    static_assert(56 * KZG_EC_MAX_UNITS <= STATS_MAX && KZG_EC_MAX_UNITS == EC_MAX_UNITS && KZG_EC_MAX_LIMBS == EC_MAX_LIMBS &&
                      KZG_EC_DIV == EC_DIV && KZG_EC_ADD == EC_ADD && KZG_EC_CHAIN == EC_CHAIN &&
                      4 * KZG_EC_MAX_LIMBS <= POLY_MAX_ROWS,
                  "the seven statistics of every unit fit the record's evaluation slots; the header's caps and modes are the "
                  "kernel's");
    Sources S;
    EcTab tab;
    memset(&tab, 0, sizeof(tab));
    const uint32_t L = curve->limbs;
    tab.n_units = n_units;
    tab.bits = curve->bits;
    tab.limbs = L;
    for (uint32_t w = 0; w < 4; w++) {
        tab.p[2 * w] = (uint32_t)curve->p[w];
        tab.p[2 * w + 1] = (uint32_t)(curve->p[w] >> 32);
        tab.a[2 * w] = (uint32_t)curve->a[w];
        tab.a[2 * w + 1] = (uint32_t)(curve->a[w] >> 32);
    }
    uint32_t inv = 1;   // p[0]^-1 mod 2^32: every round doubles the correct low bits (p odd: one is right at the start)
    for (int k = 0; k < 5; k++) inv *= 2u - tab.p[0] * inv;
    tab.n0inv = 0u - inv;
    tab.r2[0] = 1;
    for (int k = 0; k < 64 * EC_WORDS; k++) {   // r2 <- 2 r2 mod p
        uint32_t c = 0, br = 0, d[EC_WORDS];
        for (int j = 0; j < EC_WORDS; j++) {
            const uint32_t top = tab.r2[j] >> 31;
            tab.r2[j] = (tab.r2[j] << 1) | c;
            c = top;
        }
        for (int j = 0; j < EC_WORDS; j++) {
            const uint64_t x = (uint64_t)tab.r2[j] - tab.p[j] - br;
            d[j] = (uint32_t)x;
            br = (uint32_t)(x >> 32) & 1u;
        }
        if (c || !br) memcpy(tab.r2, d, sizeof(d));
    }
    for (uint32_t u = 0; u < n_units; u++) {
        const kzg_ec_unit& in = units[u];
        EcUnit& U = tab.u[u];
        U.mode = in.mode;
        U.cols = in.cols;
        U.flags = in.flags & KZG_EC_IMM_B ? EC_F_IMM_B : 0u;
        for (uint32_t w = 0; w < 4; w++) {
            U.imm[2 * w] = (uint32_t)in.imm[w];
            U.imm[2 * w + 1] = (uint32_t)(in.imm[w] >> 32);
            if (in.in[w] == KZG_EC_ABSENT) continue;
            for (uint32_t l = 0; l < L; l++) U.slot[w][l] = (uint8_t)S.slot_of(inputs.r[in.in[w] + l]);
        }
        if (in.mode == KZG_EC_CHAIN) U.opv = S.slot_of(inputs.r[in.op]);
        if (in.flags & KZG_EC_CHECK)
            for (uint32_t k = 0; k < 3; k++)
                if (in.cols >> k & 1u)
                    for (uint32_t l = 0; l < L; l++) U.exp[k][l] = (uint8_t)S.slot_of(inputs.r[in.expect[k] + l]);
    }
    uint32_t *src, *outv;
    if (int rc = units_workspace(ctx, A, F, S, n_out, 32, &src, &outv)) return rc;
    uint64_t* st = units_stats(F);
    sources_transform(ctx, A, F, S, src);
    if (int rc = units_stats_clear(ctx, A, st, n_units, 4, 3)) return rc;
    tab.src = src;
    if (int rc = assign_outputs(
            ctx, A, F, tab, n_units, outv,
            [&](uint32_t u) { return units[u].flags & KZG_EC_CHECK ? 0u : (uint32_t)__builtin_popcount(units[u].cols) * L; },
            [](uint32_t) { return false; }))
        return rc;
    {
        Span sp(ctx, A, KZG_T_POLY);
        launch_ec(A.stream, tab, T, n, st);
    }
    return units_finish(ctx, H, i, F, outv, n_out, 56 * n_units, out_c48, out_stats);
}

// The native twisted-Edwards columns (kzg_rows_commit_edwards), in the builders' frame:
//   step                      launches                         per call
//   every unit, phase 1       launch_edwards (k_edwards)       ONE, grid y = unit: numerators or projective X, Y, and Q
//   the denominators          launch_fr_batch_inv              ONE, over the (units with output) T elements of Q
//   finish                    launch_edwards_finish            ONE, grid y = output row: out <- out W
// The outputs lie side by side behind the sources in the order of the set (unit by unit, then the unit's out order), so output
// row c is vector c; behind them the denominators Q, one slice of T per unit with output, and the inversion's result W of the
// same shape.  k_edwards writes every element of Q (Montgomery 1 on an exceptional row and on the rows >= n), so the inversion
// meets no zero; its flag is read back with the statistics all the same.  The five statistics of every unit are u64 words
// behind the first two evaluation slots of the record (the inversion's scratch and flag) and come back in the copy behind the
// MSM.  With n_out = 0 (checks alone) nothing is inverted or transformed back and no MSM runs.
// Workspace: distinct sources + n_out + 2 (units with output) vectors of T, and the inversion's scan scratch in hbuf and hnext.
int rows_edwards_dev(kzg_ctx* ctx, LaneHold& H, uint32_t i, const RowTab& inputs, const kzg_edwards_curve* curve,
                     uint32_t n_units, const kzg_edwards_unit* units, uint32_t n_out, uint64_t T, uint32_t* dst, uint8_t* out_c48,
                     uint64_t* out_stats, const Blind* lay) {
    Lane& A = H.L();
    Cols F;
    if (int rc = cols_begin(ctx, A, T, lay, dst, F)) return rc;
    const uint64_t vw = F.vw, n = F.n;
    static_assert(40 * KZG_EDWARDS_MAX_UNITS <= STATS_MAX && KZG_EDWARDS_MAX_UNITS == EDW_MAX_UNITS && KZG_EDWARDS_ADD == EDW_ADD &&
                      KZG_EDWARDS_CHAIN == EDW_CHAIN,
                  "the five statistics of every unit fit the record's evaluation slots; the header's caps and modes are the "
                  "kernel's");
    Sources S;
    EdwTab tab;
    EdwFin fin;
    memset(&tab, 0, sizeof(tab));
    memset(&fin, 0, sizeof(fin));
    auto words = [](uint32_t* w, const uint8_t* be32) {   // 8 little-endian words of a 32-byte big-endian integer
        for (int k = 0; k < 8; k++)
            w[k] = (uint32_t)be32[31 - 4 * k] | (uint32_t)be32[30 - 4 * k] << 8 | (uint32_t)be32[29 - 4 * k] << 16 |
                   (uint32_t)be32[28 - 4 * k] << 24;
    };
    tab.n_units = n_units;
    words(tab.a, curve->a_be32);
    words(tab.d, curve->d_be32);
    uint32_t n_q = 0, col[EDW_MAX_UNITS][2] = {}, qof[EDW_MAX_UNITS] = {};
    bool commits[EDW_MAX_UNITS] = {};
    for (uint32_t u = 0, c = 0; u < n_units; u++) {
        const kzg_edwards_unit& in = units[u];
        EdwUnit& U = tab.u[u];
        U.mode = in.mode;
        U.cols = in.cols;
        const uint32_t n_in = in.mode == KZG_EDWARDS_ADD ? 4u : 2u;
        for (uint32_t w = 0; w < n_in; w++) {
            if (in.in[w] == KZG_EDWARDS_IMM) {
                U.slot[w] = EDW_IMM;
                words(U.imm[w], in.imm_be32[w]);
            } else {
                U.slot[w] = (uint8_t)S.slot_of(inputs.r[in.in[w]]);
            }
        }
        if (in.mode == KZG_EDWARDS_CHAIN) U.opv = S.slot_of(inputs.r[in.op]);
        if (in.flags & KZG_EDWARDS_CHECK) {
            for (uint32_t k = 0; k < 2; k++)
                if (in.cols >> k & 1u) U.exp[k] = (uint8_t)S.slot_of(inputs.r[in.expect[k]]);
            continue;
        }
        commits[u] = true;
        qof[u] = n_q++;
        for (uint32_t j = 0; j < 2 && in.out_order[j] != KZG_EDWARDS_ABSENT; j++) {
            fin.wq[c] = (uint8_t)qof[u];
            col[u][in.out_order[j]] = c++ + 1;   // (0: the name is not an output)
        }
    }
    uint32_t *src, *outv;
    if (int rc = units_workspace(ctx, A, F, S, n_out, 2 * (size_t)n_q * T * 32 + 32, &src, &outv)) return rc;
    if (n_q) {
        HIPCHK(ctx, A.hbuf.ensure(poly_level_words(n_q * T) * 4));
        HIPCHK(ctx, A.hnext.ensure(poly_level_words(n_q * T) * 4));
    }
    uint32_t *Q = outv + n_out * vw, *W = Q + n_q * vw;
    uint8_t* rec = F.rec;
    uint64_t* st = units_stats(F);
    sources_transform(ctx, A, F, S, src);
    HIPCHK(ctx, hipMemsetAsync(rec + MR_EVAL, 0, CNT_OFF + 24 * (size_t)n_units, A.stream));
    HIPCHK(ctx, hipMemsetAsync(st + 3 * n_units, 0xff, 16 * (size_t)n_units, A.stream));   // KZG_EDWARDS_NONE
    tab.src = src;
    for (uint32_t u = 0; u < n_units; u++) {
        if (!commits[u]) continue;
        tab.u[u].q = Q + qof[u] * vw;
        for (uint32_t k = 0; k < 2; k++)
            if (col[u][k]) tab.u[u].out[k] = outv + (col[u][k] - 1) * vw;
    }
    fin.out = outv;
    fin.W = W;
    {
        Span sp(ctx, A, KZG_T_POLY);
        launch_edwards(A.stream, tab, T, n, st);
        if (n_q) {
            launch_fr_batch_inv(A.stream, Q, W, nullptr, W, n_q * T, A.hbuf.as<uint32_t>(), A.hnext.as<uint32_t>(), rec + MR_EVAL,
                                reinterpret_cast<uint32_t*>(rec + MR_EVAL + 32));
            launch_edwards_finish(A.stream, fin, n_out, T, n);
        }
    }
    if (int rc = units_finish(ctx, H, i, F, outv, n_out, 40 * n_units, out_c48, out_stats)) return rc;
    uint32_t zf;
    memcpy(&zf, F.ev + 32, 4);
    if (n_q && zf) return fail(ctx, KZG_E_HIP, "edwards: the batched inversion met a zero behind k_edwards");
    return KZG_OK;
}

// The expression columns (kzg_rows_commit_expr): a set built FROM sets, every output row plain arithmetic in source rows.
// Each DISTINCT source row (by device pointer: two indices of a repeated handle name one row) that some term names is
// transformed forward once into its own vector of the lane's quotient workspace; a row no term names is not transformed.
//   step                      launches                         per call
//   forward transforms        launch_fr_ntt                    one per distinct source row named
//   evaluate + count          launch_expr (k_expr)             one per expression; a check stores nothing
//   tail                      launch_sort_tail                 one per committed expression, with `usable` only
//   inverse transform         row_to_coeffs                    one per committed expression, straight into dst
//   commit                    multi_msms_finish                ONE pass of n_out scalar sets
// A committed expression is evaluated into ONE scratch vector, takes the caller's tail behind `usable` (no closing row) and is
// transformed straight into the new set's buffer `dst`; the scratch vector is reused, the stream orders the work.  The counts
// and first indices are u64 words behind the first two evaluation slots of the record (the inversion's slots of the derived
// call, so that the layouts agree) and come back in the copy behind the MSM: the call never waits on its own.  With n_out = 0
// nothing is transformed back and no MSM runs: the record's one copy and its synchronisation are all that is left.
// Workspace: distinct sources + 1 vectors of T.
int rows_expr_dev(kzg_ctx* ctx, LaneHold& H, uint32_t i, const RowTab& inputs, uint32_t n_exprs, const ExprPlan* exprs,
                  const uint8_t* is_check, uint32_t n_out, uint64_t T, uint32_t* dst, uint8_t* out_c48, uint64_t* out_nonzero,
                  uint64_t* out_first, const Blind* lay) {
    Lane& A = H.L();
    Cols F;
    if (int rc = cols_begin(ctx, A, T, lay, dst, F)) return rc;
    const uint64_t vw = F.vw, n = F.n;
    static_assert(16 * KZG_MAX_BATCH_OPEN <= STATS_MAX && KZG_MAX_BATCH_OPEN <= POLY_MAX_ROWS,
                  "the count and the first index of every expression fit the record's evaluation slots");
    static_assert(KZG_MAX_GATE_TERMS == EXPR_MAX_TERMS && KZG_MAX_EXPR_FACTORS == EXPR_MAX_FACTORS, "the header's caps are the kernel's");
    Sources S;
    ExprPlan plan[KZG_MAX_BATCH_OPEN];
    for (uint32_t e = 0; e < n_exprs; e++) {
        plan[e] = exprs[e];
        plan_sources(plan[e], inputs, S);
    }
    HIPCHK(ctx, A.qext.ensure(((size_t)S.nd + 1) * T * 32));
    uint32_t *src = A.qext.as<uint32_t>(), *scratch = src + S.nd * vw;
    uint64_t *cnt = reinterpret_cast<uint64_t*>(F.rec + MR_EVAL + CNT_OFF), *first = cnt + n_exprs;
    RowTab st;
    memset(&st, 0, sizeof(st));
    sources_transform(ctx, A, F, S, src);
    for (uint32_t d = 0; d < S.nd; d++) st.r[d] = src + d * vw;
    HIPCHK(ctx, hipMemsetAsync(cnt, 0, 8 * (size_t)n_exprs, A.stream));
    HIPCHK(ctx, hipMemsetAsync(first, 0xff, 8 * (size_t)n_exprs, A.stream));   // KZG_EXPR_NONE
    for (uint32_t e = 0, c = 0; e < n_exprs; e++) {
        {
            Span sp(ctx, A, KZG_T_POLY);
            launch_expr(A.stream, st, plan[e], is_check[e] ? nullptr : scratch, T, n, cnt + e, first + e);
        }
        if (is_check[e]) continue;
        if (int rc = emit_column(ctx, A, F, scratch, c++)) return rc;
    }
    const uint8_t* stats;
    if (int rc = stats_finish(ctx, H, i, F, n_out, 16 * n_exprs, out_c48, &stats)) return rc;
    memcpy(out_nonzero, stats, 8 * (size_t)n_exprs);
    memcpy(out_first, stats + 8 * (size_t)n_exprs, 8 * (size_t)n_exprs);
    return KZG_OK;
}

// The first-order recurrence columns (kzg_rows_commit_recurrence): a set built FROM sets, every output column a running value
// v[t + 1] = A[t] v[t] + B[t] whose multiplier A and addend B are expressions in source rows.  Sources as in rows_expr_dev: each
// DISTINCT source row that some term names is transformed forward once.
//   step                      launches                         per call
//   forward transforms        launch_fr_ntt                    one per distinct source row named
//   A and B                   launch_expr (k_expr, unchanged)  two per recurrence; an empty side is the constant 1 / 0
//   the scan                  launch_recur_scan                K folds, one top kernel, K walks per recurrence
//   tail                      launch_blind_tail                one per recurrence, with `usable` < T - 1 only
//   inverse transform         row_to_coeffs                    one per recurrence, straight into dst
//   commit                    multi_msms_finish                ONE pass of n_recs scalar sets
// A, B and the output are three scratch vectors that every recurrence reuses; the stream orders the work.  The scan writes the
// closing value of recurrence c into evaluation slot c of the record (and, in the usable layout, into row `usable` of the
// output); the closings come back in the record's copy behind the MSM: the call never waits on its own.  launch_expr's two
// counters go to two spare words behind the last closing slot and are not read.
// Workspace: distinct sources + 3 vectors of T, and 2 recur_level_elems(n) elements of level scratch.
int rows_recur_dev(kzg_ctx* ctx, LaneHold& H, uint32_t i, const RowTab& inputs, uint32_t n_recs, const RecurSpec* recs, uint64_t T,
                   uint32_t* dst, uint8_t* out_c48, uint8_t* out_closing32, const Blind* lay) {
    Lane& A = H.L();
    Cols F;
    if (int rc = cols_begin(ctx, A, T, lay, dst, F)) return rc;
    const uint64_t vw = F.vw, n = F.n;   // n: the steps of the recurrence, rows 0 .. n - 1 are v[0] .. v[n - 1]
    constexpr uint32_t DUMP_OFF = 32 * KZG_MAX_BATCH_OPEN;   // launch_expr's counters, behind the closings
    static_assert(DUMP_OFF + 16 <= MR_PAIRS * 32 && KZG_MAX_BATCH_OPEN <= POLY_MAX_ROWS,
                  "the closing of every recurrence and the two spare words fit the record's evaluation slots");
    static_assert(KZG_MAX_GATE_TERMS == EXPR_MAX_TERMS && KZG_MAX_EXPR_FACTORS == EXPR_MAX_FACTORS, "the header's caps are the kernel's");
    static const uint8_t ONE_BE[32] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1};
    static const uint8_t ZERO_BE[32] = {};
    Sources S;
    ExprPlan plan[KZG_MAX_BATCH_OPEN][2];
    for (uint32_t e = 0; e < n_recs; e++)
        for (int side = 0; side < 2; side++) {
            ExprPlan& pl = plan[e][side];
            pl = side ? recs[e].add : recs[e].mul;
            if (pl.n_terms == 0) {   // the empty side: the constant 1 (A) or 0 (B), one term without factors
                memset(&pl, 0, sizeof pl);
                pl.n_terms = 1;
                pl.coeffs_be32 = side ? ZERO_BE : ONE_BE;
            }
            plan_sources(pl, inputs, S);
        }
    HIPCHK(ctx, A.qext.ensure(((size_t)S.nd + 3) * T * 32));
    HIPCHK(ctx, A.hbuf.ensure(recur_level_elems(n) * 32));
    HIPCHK(ctx, A.hnext.ensure(recur_level_elems(n) * 32));
    uint32_t *src = A.qext.as<uint32_t>(), *va = src + S.nd * vw, *vb = va + vw, *out = vb + vw;
    uint8_t* rec = F.rec;
    uint64_t* dump = reinterpret_cast<uint64_t*>(rec + MR_EVAL + DUMP_OFF);
    RowTab st;
    memset(&st, 0, sizeof(st));
    sources_transform(ctx, A, F, S, src);
    for (uint32_t d = 0; d < S.nd; d++) st.r[d] = src + d * vw;
    HIPCHK(ctx, hipMemsetAsync(dump, 0, 16, A.stream));
    for (uint32_t e = 0; e < n_recs; e++) {
        {
            Span sp(ctx, A, KZG_T_POLY);
            launch_expr(A.stream, st, plan[e][0], va, T, n, dump, dump + 1);
            launch_expr(A.stream, st, plan[e][1], vb, T, n, dump, dump + 1);
            launch_recur_scan(A.stream, va, vb, n, A.hbuf.as<uint32_t>(), A.hnext.as<uint32_t>(), recs[e].start_be32, out,
                              rec + MR_EVAL + 32 * e, lay ? out + 8 * n : nullptr);
            if (lay) launch_blind_tail(A.stream, out, T, n, lay->tail_be32 + 32 * (size_t)e * (T - n - 1), A.flags());
        }
        const uint32_t* cf;
        if (int rc = row_to_coeffs(ctx, A, out, T, 1, &cf, dst + e * vw)) return rc;
    }
    HIPCHK(ctx, hipGetLastError());
    return multi_msms_finish(ctx, H, i, T, dst, n_recs, 0, n_recs, out_c48, out_closing32, nullptr);
}

// The fetched columns (kzg_rows_commit_fetch): a set built FROM sets, every output cell a table cell READ by the key (or the
// row index) that the input columns hold.  The w_tab table columns are transformed forward once into w_tab vectors of the
// lane's quotient workspace; with n_keys >= 1 the join of rows_multiplicities_dev is built over the first n_keys of them
// (launch_join_build / _rows with w = n_keys, unchanged), the others are the payload.
//   step                      launches                               per call
//   forward transforms        launch_fr_ntt                          w_tab, then max(n_keys, 1) per read
//   build                     launch_join_build(_rows)               one (n_keys >= 1)
//   fetch + count             launch_join_fetch / launch_fetch_index one per read, into n_per = index + n_pay vectors
//   tail                      launch_sort_tail                       one per output column, with `usable` only
//   inverse transform         row_to_coeffs                          one per output column, straight into dst
//   commit                    multi_msms_finish                      ONE pass of n_reads n_per scalar sets
// The input vectors and the n_per output vectors are reused by every read; the stream orders the work.  The counts and first
// indices are u64 words behind the first two evaluation slots of the record (the layout of rows_expr_dev), the join's overrun
// word lies in the second slot; all come back in the copy behind the MSM: the call never waits on its own.
// Workspace: w_tab + max(n_keys, 1) + n_per vectors of T, and 2 T u32 slots in the staging buffer (n_keys >= 1).
int rows_fetch_dev(kzg_ctx* ctx, LaneHold& H, uint32_t i, const RowTab& inputs, const RowTab& table, uint32_t n_reads,
                   uint32_t n_keys, uint32_t w_tab, bool index, uint64_t T, uint32_t* dst, uint8_t* out_c48, uint64_t* out_missing,
                   uint64_t* out_first, bool* out_overrun, const Blind* lay) {
    Lane& A = H.L();
    Cols F;
    if (int rc = cols_begin(ctx, A, T, lay, dst, F)) return rc;
    const uint64_t vw = F.vw, n = F.n;   // n: the cells that are read and the table rows that can answer
    const uint32_t n_in = n_keys ? n_keys : 1, n_pay = w_tab - n_keys, n_per = n_pay + (index ? 1u : 0u), n_out = n_reads * n_per;
    const uint32_t cap = (uint32_t)(2 * T);           // slots: a power of two, load <= 1 / 2 (T <= 2^27: the caller)
    constexpr uint32_t OVR_OFF = 32;                  // the overrun word, in front of the counts and the first indices
    static_assert(16 * KZG_MAX_BATCH_OPEN <= STATS_MAX && KZG_MAX_BATCH_OPEN <= POLY_MAX_ROWS,
                  "the count and the first index of every read fit the record's evaluation slots");
    HIPCHK(ctx, A.qext.ensure(((size_t)w_tab + n_in + n_per) * T * 32));
    if (n_keys) HIPCHK(ctx, A.qstage.ensure((size_t)cap * 4));
    uint32_t *tab = A.qext.as<uint32_t>(), *in = tab + (uint64_t)w_tab * vw, *out = in + (uint64_t)n_in * vw;
    uint32_t* slots = n_keys ? A.qstage.as<uint32_t>() : nullptr;
    uint8_t* rec = F.rec;
    uint64_t *cnt = reinterpret_cast<uint64_t*>(rec + MR_EVAL + CNT_OFF), *first = cnt + n_reads;
    uint32_t* overrun = reinterpret_cast<uint32_t*>(rec + MR_EVAL + OVR_OFF);
    for (uint32_t c = 0; c < w_tab; c++) {
        Span sp(ctx, A, KZG_T_NTT);
        launch_fr_ntt(A.stream, table.r[c], tab + c * vw, F.lg, F.tw, nullptr, F.mid);
    }
    {
        Span sp(ctx, A, KZG_T_POLY);
        HIPCHK(ctx, hipMemsetAsync(rec + MR_EVAL, 0, CNT_OFF + 8 * (size_t)n_reads, A.stream));
        HIPCHK(ctx, hipMemsetAsync(first, 0xff, 8 * (size_t)n_reads, A.stream));   // KZG_FETCH_NONE
        if (n_keys) {
            HIPCHK(ctx, hipMemsetAsync(slots, 0xff, (size_t)cap * 4, A.stream));
            // usable: only the table rows below it enter the join, so no row at or behind it can answer
            if (lay) launch_join_build_rows(A.stream, tab, T, n, n_keys, slots, cap, overrun);
            else launch_join_build(A.stream, tab, T, n_keys, slots, cap, overrun);
        }
    }
    for (uint32_t l = 0, c = 0; l < n_reads; l++) {
        for (uint32_t k = 0; k < n_in; k++) {
            Span sp(ctx, A, KZG_T_NTT);
            launch_fr_ntt(A.stream, inputs.r[l * n_in + k], in + k * vw, F.lg, F.tw, nullptr, F.mid);
        }
        {
            Span sp(ctx, A, KZG_T_POLY);
            if (n_keys) launch_join_fetch(A.stream, tab, in, T, n, n_keys, n_pay, index, slots, cap, out, cnt + l, first + l, overrun);
            else launch_fetch_index(A.stream, tab, in, T, n, n_pay, out, cnt + l, first + l);
        }
        for (uint32_t p = 0; p < n_per; p++, c++)
            if (int rc = emit_column(ctx, A, F, out + p * vw, c)) return rc;
    }
    const uint8_t* stats;
    if (int rc = stats_finish(ctx, H, i, F, n_out, 16 * n_reads, out_c48, &stats)) return rc;
    uint32_t of;
    memcpy(&of, F.ev + OVR_OFF, 4);
    *out_overrun = of != 0;
    memcpy(out_missing, stats, 8 * (size_t)n_reads);
    memcpy(out_first, stats + 8 * (size_t)n_reads, 8 * (size_t)n_reads);
    return KZG_OK;
}

// the quotient's constants of one (T, E), shared by all lanes like the twiddles: built once under the ctx mutex
static int ensure_quot_consts(kzg_ctx* ctx, Lane& L, int log_t, int ext_log, const uint32_t* tw_n, const uint32_t** qc) {
    std::lock_guard<std::mutex> lk(ctx->mu);
    const int key = log_t * 4 + ext_log;
    if (!ctx->quot_consts.count(key)) {
        DevBuf b;
        HIPCHK(ctx, b.ensure(quot_consts_elems(log_t, ext_log) * 32));
        launch_quot_consts(L.stream, b.as<uint32_t>(), log_t, ext_log, tw_n);
        HIPCHK(ctx, hipStreamSynchronize(L.stream));
        ctx->quot_consts[key] = std::move(b);
    }
    *qc = ctx->quot_consts[key].as<uint32_t>();
    return KZG_OK;
}
// The PLONK quotient (kzg_rows_commit_quotient): a set built FROM sets.  Every DISTINCT row the constraints name (by device
// pointer: a wire is named by the gate and by the permutation) is extended to the coset g H_N, N = E T -- one scaling launch
// into the lane's staging vector, one forward transform of length N into its own vector of the lane's quotient workspace --
// and so is L_0 when there is a permutation or a lookup part (a rotated factor reads the SAME vector at another index: no
// vector and no transform of its own); one pointwise launch writes num / Z_H into the staging vector; the inverse
// transform and the g^-i launch leave the P pieces in the new set's buffer `dst` and OR the coefficients above P T into the
// record's first evaluation slot; ONE MSM pass of P scalar sets commits.  Workspace: (distinct rows + 2) vectors of N.
// The flag travels in the record's one copy behind the MSM, so an instance that fails the shape check still pays the MSM
// before KZG_E_ARG comes back: no set is created, but the error path is not a fast path (a read-back of its own in front of
// the MSM would cost every good call a synchronisation).
// The front half, shared with kzg_rows_quotient_part: the extensions and the pointwise launch, which leaves num / Z_H on the
// coset (N canonical elements) in the lane's staging vector.
static int quot_front(kzg_ctx* ctx, Lane& A, const RowTab& rt, uint32_t n_rows, uint64_t T, const QuotPlan& qp) {
    const int lg = ilog2_exact(T), ext_log = (int)qp.ext_log, lgn = lg + ext_log;
    const uint64_t N = T << ext_log, nw = N * 8;   // one extended vector, in words
    uint32_t *tw = nullptr, *twi = nullptr, *invn = nullptr;
    if (int rc = ensure_twiddles(ctx, A, lgn, 0, &tw, nullptr)) return rc;
    if (int rc = ensure_twiddles(ctx, A, lgn, 1, &twi, &invn)) return rc;
    const uint32_t* qc = nullptr;
    if (int rc = ensure_quot_consts(ctx, A, lg, ext_log, tw, &qc)) return rc;
    // the rows in use, one workspace vector per distinct device pointer
    bool used[POLY_MAX_ROWS] = {};
    for (uint32_t u = 0; u < qp.n_terms; u++)
        for (uint32_t f = 0; f < qp.term_len[u]; f++) used[qp.term_row[u][f]] = true;
    for (uint32_t j = 0; j < qp.k; j++) used[qp.wire[j]] = used[qp.sigma[j]] = true;
    if (qp.k) used[qp.z_row] = true;
    for (uint32_t j = 0; j < qp.n_lookups * qp.width; j++) used[qp.in_row[j]] = true;
    for (uint32_t j = 0; qp.n_lookups && j < qp.width; j++) used[qp.tab_row[j]] = true;
    if (qp.n_lookups) used[qp.mult_row] = used[qp.sum_row] = true;
    if (qp.active && (qp.k || qp.n_lookups)) used[qp.active_row] = true;   // A: one more distinct row (a factor of P1 and LK1)
    if (qp.link) used[qp.link_row] = true;                                 // f_prev of a linked P2
    for (uint32_t l = 0; qp.sel && l < qp.n_lookups; l++)                 // q_l: extended once like any row the part names
        if (qp.sel_row[l] != 0xffu) used[qp.sel_row[l]] = true;
    const bool need_l0 = qp.k || qp.n_lookups;   // P2 and LK2
    int slot[POLY_MAX_ROWS];
    uint32_t nd = 0;
    for (uint32_t j = 0; j < n_rows; j++) {
        slot[j] = -1;
        if (!used[j]) continue;
        for (uint32_t e = 0; e < j && slot[j] < 0; e++)
            if (used[e] && rt.r[e] == rt.r[j]) slot[j] = slot[e];
        if (slot[j] < 0) slot[j] = (int)nd++;
    }
    HIPCHK(ctx, A.qext.ensure((size_t)std::max(nd + (need_l0 ? 1u : 0u), 1u) * N * 32));   // (constant terms alone: no row)
    HIPCHK(ctx, A.qstage.ensure(N * 32));
    HIPCHK(ctx, A.ntt_mid.ensure(N * 48));
    uint32_t *ext = A.qext.as<uint32_t>(), *stage = A.qstage.as<uint32_t>(), *mid = A.ntt_mid.as<uint32_t>();
    RowTab et;
    memset(&et, 0, sizeof(et));
    for (uint32_t j = 0, done = 0; j <= n_rows; j++) {   // (j == n_rows: L_0)
        uint32_t* vec;
        if (j < n_rows) {
            if (slot[j] < 0) continue;
            vec = ext + (uint64_t)slot[j] * nw;
            et.r[j] = vec;
            if ((uint32_t)slot[j] < done) continue;   // a repeated row: transformed already
            done++;
        } else {
            if (!need_l0) break;
            vec = ext + (uint64_t)nd * nw;
        }
        {
            Span sp(ctx, A, KZG_T_POLY);
            launch_quot_extend(A.stream, j < n_rows ? rt.r[j] : nullptr, stage, lg, ext_log, qc);
        }
        Span sp(ctx, A, KZG_T_NTT);
        launch_fr_ntt(A.stream, stage, vec, lgn, tw, nullptr, mid);
    }
    Span sp(ctx, A, KZG_T_POLY);
    launch_quot_points(A.stream, et, ext + (uint64_t)nd * nw, stage, lg, qp, tw, qc, A.flags());
    return KZG_OK;
}
// The back half, which is kzg_rows_quotient_finish over the accumulator: `src` (num / Z_H on the coset, N canonical elements, only read) through
// the inverse transform into the lane's quotient workspace, the g^-i launch with the shape check, the one MSM pass.
int rows_quotient_finish_dev(kzg_ctx* ctx, LaneHold& H, uint32_t i, uint64_t T, int ext_log, const uint32_t* src, uint32_t n_pieces,
                     uint32_t* dst, uint8_t* out_c48, bool* out_bad_shape) {
    Lane& A = H.L();
    if (int rc = ensure_multi_record(ctx, A)) return rc;
    const int lg = ilog2_exact(T), lgn = lg + ext_log;
    const uint64_t N = T << ext_log;
    uint32_t *tw = nullptr, *twi = nullptr, *invn = nullptr;
    if (int rc = ensure_twiddles(ctx, A, lgn, 0, &tw, nullptr)) return rc;
    if (int rc = ensure_twiddles(ctx, A, lgn, 1, &twi, &invn)) return rc;
    const uint32_t* qc = nullptr;
    if (int rc = ensure_quot_consts(ctx, A, lg, ext_log, tw, &qc)) return rc;
    HIPCHK(ctx, A.qext.ensure(N * 32));
    HIPCHK(ctx, A.ntt_mid.ensure(N * 48));
    uint32_t *ext = A.qext.as<uint32_t>(), *mid = A.ntt_mid.as<uint32_t>();
    uint8_t* rec = A.brec.as<uint8_t>();
    HIPCHK(ctx, hipMemsetAsync(rec + MR_EVAL, 0, 32, A.stream));
    {
        Span sp(ctx, A, KZG_T_NTT);
        launch_fr_ntt(A.stream, src, ext, lgn, twi, invn, mid);
    }
    {
        Span sp(ctx, A, KZG_T_POLY);
        launch_quot_pieces(A.stream, ext, dst, lg, ext_log, n_pieces, qc, reinterpret_cast<uint32_t*>(rec + MR_EVAL));
    }
    uint8_t ev[32];
    if (int rc = multi_msms_finish(ctx, H, i, T, dst, n_pieces, 0, 1, out_c48, ev, nullptr)) return rc;
    uint32_t tf;
    memcpy(&tf, ev, 4);
    *out_bad_shape = tf != 0;
    return KZG_OK;
}
int rows_quotient_dev(kzg_ctx* ctx, LaneHold& H, uint32_t i, const RowTab& rt, uint32_t n_rows, uint64_t T, const QuotPlan& qp,
                      uint32_t n_pieces, uint32_t* dst, uint8_t* out_c48, bool* out_bad_shape) {
    Lane& A = H.L();
    if (int rc = quot_front(ctx, A, rt, n_rows, T, qp)) return rc;
    return rows_quotient_finish_dev(ctx, H, i, T, (int)qp.ext_log, A.qstage.as<uint32_t>(), n_pieces, dst, out_c48, out_bad_shape);
}
// kzg_rows_quotient_part in two steps, so that the caller can take the accumulator's mutex between them.  The front half
// leaves the part's num / Z_H in the lane's staging vector; the add is acc (+)= scale * that vector, the call's LAST device
// step, and ends the call (the stream is drained on any failure: nothing of this call touches the accumulator afterwards).
// Every scalar was range-checked on the host, so finish() cannot answer KZG_E_SCALAR here; the caller nevertheless treats any
// failure behind the add's launch as "contents unknown".
int rows_quotient_front_dev(kzg_ctx* ctx, LaneHold& H, const RowTab& rt, uint32_t n_rows, uint64_t T, const QuotPlan& qp) {
    return quot_front(ctx, H.L(), rt, n_rows, T, qp);
}
int rows_quotient_add_dev(kzg_ctx* ctx, LaneHold& H, uint64_t T, uint32_t ext_log, const uint8_t* scale_be32, uint32_t* acc,
                          bool first) {
    Lane& A = H.L();
    {
        Span sp(ctx, A, KZG_T_POLY);
        launch_quot_accumulate(A.stream, acc, A.qstage.as<uint32_t>(), T << ext_log, scale_be32, first);
    }
    if (int rc = finish(ctx, A)) {
        (void)hipStreamSynchronize(A.stream);
        (void)hipGetLastError();
        return rc;
    }
    H.clean = true;
    return KZG_OK;
}

}  // namespace kzg_impl
