// serve.hip -- the serving entry points of the C-ABI: commit / open / commit+open of a worker row (host bytes, cached
// two-call route, resident slot), plain and partial MSMs, tickets, NTT / evaluation for the validator side, sums of points,
// calibration.  Each one names the reference call it replaces in include/kzg_mi355x.h; the kernel sequences are pipeline.hip.
#include "ctx.hip.h"

using namespace kzg_impl;

extern "C" {

static int msm_host_common(kzg_ctx* ctx, const uint8_t* scalars_be32, uint64_t n, uint64_t srs_offset, uint8_t* out,
                           bool partial) {
    if (!ctx || !out || (n && !scalars_be32)) return KZG_E_ARG;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    LaneHold H(ctx);
    if (int rc = H.take()) return rc;
    Lane& L = H.L();
    int rc = need_srs(ctx);
    if (rc) return rc;
    prof_begin(ctx, L);
    rc = clear_flags(ctx, L);
    if (rc) return rc;
    HIPCHK(ctx, L.scal.ensure(n * 32 + 32));
    rc = upload_fr(ctx, L, scalars_be32, n, L.scal.as<uint32_t>(), 0);
    if (rc) return rc;
    rc = msm_core(ctx, L, ScalarSets::one(L.scal.as<uint32_t>(), 0), n, srs_offset, L.res());
    if (rc) return rc;
    if (partial) queue_pack(ctx, L);
    else queue_encode(ctx, L, true, false);
    rc = finish(ctx, L);
    if (rc) return rc;
    if (partial) result_partial(ctx, L, out);
    else result_c48(ctx, L, 0, out);
    H.clean = true;
    return KZG_OK;
}
int kzg_msm(kzg_ctx* ctx, const uint8_t* scalars_be32, uint64_t n, uint64_t srs_offset, uint8_t out48[48]) {
    return msm_host_common(ctx, scalars_be32, n, srs_offset, out48, false);
}
int kzg_msm_partial(kzg_ctx* ctx, const uint8_t* scalars_be32, uint64_t n, uint64_t srs_offset,
                    uint8_t out_xyzz192[192]) {
    return msm_host_common(ctx, scalars_be32, n, srs_offset, out_xyzz192, true);
}

// Sums of a few points run on their own stream and buffers: legal while MSM tickets are outstanding (a rank sums the
// gathered partials of step i while its step i+1 is already on the GPU).  Three input forms:
//   host partials (192-byte XYZZ records), device partials (the output tensor of an all_gather; every prior writer has
//   completed), and 48-byte compressed points (the commitments of the worker rows: Pianist's master aggregation
//   sum_i commit_i, reference neurons/validator.py:196-198, README.md:38) which are decompressed on the GPU.
static int g1_sum_common(kzg_ctx* ctx, const uint8_t* in, uint32_t count, uint8_t out48[48], int form) {
    if (!ctx || !out48 || (count && !in)) return KZG_E_ARG;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    std::lock_guard<std::mutex> lk(ctx->aux_mu);
    const size_t rec = form == 2 ? 48 : 192;
    HIPCHK(ctx, ctx->aux_in.ensure((size_t)count * rec + 192));
    HIPCHK(ctx, ctx->aux_pts.ensure(((size_t)count + 2) * sizeof(g1_xyzz_t)));
    HIPCHK(ctx, ctx->aux_out.ensure(256));
    hipStream_t s = ctx->aux;
    g1_xyzz_t* pts = ctx->aux_pts.as<g1_xyzz_t>();
    uint32_t* bad = ctx->aux_out.as<uint32_t>() + 32;
    HIPCHK(ctx, hipMemsetAsync(bad, 0, 4, s));
    if (form == 2) {
        static_assert(sizeof(g1_affine_t) <= sizeof(g1_xyzz_t), "affine rows are staged in the XYZZ scratch");
        if (count) HIPCHK(ctx, hipMemcpyAsync(ctx->aux_in.p, in, (size_t)count * 48, hipMemcpyHostToDevice, s));
        g1_affine_t* aff = reinterpret_cast<g1_affine_t*>(pts + 1);
        launch_srs_from_c48(s, ctx->aux_in.as<uint8_t>(), aff, count, bad);
        // these are UNTRUSTED points (miners' commitments): on the curve is not enough, E(Fp) has a 2^126 cofactor
        launch_g1_subgroup_check(s, aff, count, bad);
        launch_g1_sum_affine(s, aff, count, pts);
    } else {
        const uint32_t* src = reinterpret_cast<const uint32_t*>(in);
        if (form == 0) {
            if (count) HIPCHK(ctx, hipMemcpyAsync(ctx->aux_in.p, in, (size_t)count * 192, hipMemcpyHostToDevice, s));
            src = ctx->aux_in.as<uint32_t>();
        }
        launch_xyzz_unpack(s, src, pts + 1, count);
        launch_g1_sum(s, pts + 1, count, pts);
    }
    uint8_t* pin = ctx->aux_pin;
    if (ctx->host_finish) {
        HIPCHK(ctx, hipMemcpyAsync(pin, pts, sizeof(g1_xyzz_t), hipMemcpyDeviceToHost, s));
    } else {
        launch_g1_compress(s, pts, ctx->aux_out.as<uint8_t>());
        HIPCHK(ctx, hipMemcpyAsync(pin, ctx->aux_out.p, 48, hipMemcpyDeviceToHost, s));
    }
    HIPCHK(ctx, hipMemcpyAsync(pin + 224, bad, 4, hipMemcpyDeviceToHost, s));
    HIPCHK(ctx, hipStreamSynchronize(s));
    HIPCHK(ctx, hipGetLastError());
    if (const uint32_t b = *reinterpret_cast<const uint32_t*>(pin + 224))
        return fail(ctx, KZG_E_POINT, (b & 3u) ? "compressed G1 input malformed, not reduced or not on the curve"
                                                : "G1 input on the curve but outside the prime-order subgroup");
    if (ctx->host_finish) kzg_host::xyzz_to_c48(reinterpret_cast<const uint32_t*>(pin), out48);
    else memcpy(out48, pin, 48);
    return KZG_OK;
}
int kzg_g1_sum(kzg_ctx* ctx, const uint8_t* partials_xyzz192, uint32_t count, uint8_t out48[48]) {
    return g1_sum_common(ctx, partials_xyzz192, count, out48, 0);
}
int kzg_g1_sum_dev(kzg_ctx* ctx, const void* dev_partials_xyzz192, uint32_t count, uint8_t out48[48]) {
    return g1_sum_common(ctx, reinterpret_cast<const uint8_t*>(dev_partials_xyzz192), count, out48, 1);
}
int kzg_g1_sum_compressed(kzg_ctx* ctx, const uint8_t* points_c48, uint32_t count, uint8_t out48[48]) {
    return g1_sum_common(ctx, points_c48, count, out48, 2);
}

static int commit_open_host(kzg_ctx* ctx, uint32_t i, const uint8_t* row_be32, uint64_t T, int evaluation_form,
                            const uint8_t* alpha, uint8_t* c48, uint8_t* e32, uint8_t* p48) {
    if (!ctx || !row_be32 || (p48 && (!alpha || !e32))) return KZG_E_ARG;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    LaneHold H(ctx);
    if (int rc = H.take()) return rc;
    Lane& L = H.L();
    int rc = check_worker(ctx, i, T);
    if (rc) return rc;
    prof_begin(ctx, L);
    rc = clear_flags(ctx, L);
    if (rc) return rc;
    HIPCHK(ctx, L.coeffA.ensure(T * 32));
    rc = upload_fr(ctx, L, row_be32, T, L.coeffA.as<uint32_t>(), 1);
    if (rc) return rc;
    return commit_open_dev(ctx, H, i, L.coeffA.as<uint32_t>(), T, evaluation_form, alpha, c48, e32, p48);
}
// ---- the UNCHANGED reference miner (neurons/miner.py:56-61) calls worker_commit(i, poly) and then worker_open(i, poly, x)
// with the same row: the second call used to decode, upload and inverse-transform it all over again.  With a content tag
// (a 128-bit keyed hash the codec folds into its decode pass) the coefficient vector of the last few rows stays on the
// device: a call whose (tag, T, form) is cached skips the INTT and keeps the upload off its critical path; anything else
// behaves exactly like the untagged call and leaves its own coefficients behind.  The tag (zkp_subnet_amd/csrc/wire_py.c:
// a keyed multiply-fold over the decoded bytes, fast but with no cryptographic analysis) is a HINT, not a proof of
// identity: every hit is verified bit for bit on the GPU against the row the slot was filled from.
static int rcache_lookup(kzg_ctx* ctx, const uint8_t tag[16], uint64_t T, int ef) { return ctx->book.rcache_lookup(tag, T, ef); }
static void rcache_release(kzg_ctx* ctx, int k, bool valid, const uint8_t tag[16], uint64_t T, int ef) {
    ctx->book.rcache_release(k, valid, tag, T, ef);
}
static int commit_open_host_cached(kzg_ctx* ctx, uint32_t i, const uint8_t* row_be32, uint64_t T, int evaluation_form,
                                   const uint8_t tag[16], const uint8_t* alpha, uint8_t* c48, uint8_t* e32, uint8_t* p48) {
    if (!ctx || !row_be32 || !tag || (p48 && (!alpha || !e32))) return KZG_E_ARG;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    LaneHold H(ctx);
    if (int rc = H.take()) return rc;
    Lane& L = H.L();
    int rc = check_worker(ctx, i, T);
    if (rc) return rc;
    prof_begin(ctx, L);
    rc = clear_flags(ctx, L);
    if (rc) return rc;
    int look = rcache_lookup(ctx, tag, T, evaluation_form);
    if (look >= 0) {
        // hit: no INTT, and nothing of the row on the request's critical path.  The tag is only a HINT: the caller's row
        // is uploaded on a side stream while the MSM runs and compared, bit for bit, with the row this slot was filled
        // from; the publish waits for that verdict.  A colliding tag costs one wasted pass, never a wrong answer.
        auto& e = ctx->rcache[look];
        const VerifyJob job{row_be32, T, e.raw.as<uint32_t>()};
        rc = commit_open_dev(ctx, H, i, nullptr, T, evaluation_form, alpha, c48, e32, p48, e.coef.as<uint32_t>(), nullptr, &job);
        if (rc != KZG_OK) H.drain();            // queued kernels may still read the slot
        const bool same = rc != KZG_OK || *reinterpret_cast<const volatile uint32_t*>(L.pin + TB_VERIFY) == 0;
        rcache_release(ctx, look, same, tag, T, evaluation_form);   // a slot whose tag collided is dropped
        if (same) return rc;
        ctx->book.rcache_collision();   // equal tags, different rows: the answer just computed belongs to the OTHER row --
                                        // discard it, take the miss path
        H.clean = false;
        prof_begin(ctx, L);
        rc = clear_flags(ctx, L);
        if (rc) return rc;
        look = -1;                              // no caching for this call (its tag is known to be ambiguous)
    }
    const int slot = look <= -2 ? -2 - look : -1;
    uint32_t* dst = nullptr;
    if (slot >= 0) {
        auto& e = ctx->rcache[slot];
        if (e.coef.ensure(T * 32) == hipSuccess && e.raw.ensure(T * 32) == hipSuccess) dst = e.coef.as<uint32_t>();
        else (void)hipGetLastError();
    }
    rc = L.coeffA.ensure(T * 32) == hipSuccess ? KZG_OK : fail(ctx, KZG_E_NOMEM, "row buffer");
    if (!rc) rc = upload_fr(ctx, L, row_be32, T, L.coeffA.as<uint32_t>(), 1);
    if (!rc && dst)   // the uploaded bytes themselves stay with the slot: what a later hit is verified against
        rc = hipMemcpyAsync(ctx->rcache[slot].raw.p, L.in_be_src, T * 32, hipMemcpyDeviceToDevice, L.stream) == hipSuccess
                 ? KZG_OK : fail(ctx, KZG_E_HIP, "row cache: copy of the uploaded row");
    if (!rc) rc = commit_open_dev(ctx, H, i, L.coeffA.as<uint32_t>(), T, evaluation_form, alpha, c48, e32, p48, nullptr, dst);
    if (rc != KZG_OK && slot >= 0) H.drain();   // a failed call may have kernels queued that still write the slot: not reusable before
    if (slot >= 0) rcache_release(ctx, slot, rc == KZG_OK && dst != nullptr, tag, T, evaluation_form);
    return rc;
}
int kzg_commit_cached(kzg_ctx* ctx, uint32_t i, const uint8_t* row_be32, uint64_t T, int evaluation_form,
                      const uint8_t content_tag[16], uint8_t out_commitment48[48]) {
    if (!out_commitment48) return KZG_E_ARG;
    return commit_open_host_cached(ctx, i, row_be32, T, evaluation_form, content_tag, nullptr, out_commitment48, nullptr, nullptr);
}
int kzg_open_cached(kzg_ctx* ctx, uint32_t i, const uint8_t* row_be32, uint64_t T, int evaluation_form,
                    const uint8_t content_tag[16], const uint8_t alpha_be32[32], uint8_t out_eval32[32],
                    uint8_t out_proof48[48]) {
    if (!out_proof48) return KZG_E_ARG;
    return commit_open_host_cached(ctx, i, row_be32, T, evaluation_form, content_tag, alpha_be32, nullptr, out_eval32, out_proof48);
}
int kzg_row_cache_stats(kzg_ctx* ctx, uint64_t out_hits_misses[2]) {
    if (!ctx || !out_hits_misses) return KZG_E_ARG;
    uint64_t st[3];
    ctx->book.rcache_stats(st);
    out_hits_misses[0] = st[0];
    out_hits_misses[1] = st[1];
    return KZG_OK;
}
int kzg_commit(kzg_ctx* ctx, uint32_t i, const uint8_t* row_be32, uint64_t T, int evaluation_form,
               uint8_t out_commitment48[48]) {
    if (!out_commitment48) return KZG_E_ARG;
    return commit_open_host(ctx, i, row_be32, T, evaluation_form, nullptr, out_commitment48, nullptr, nullptr);
}
int kzg_open(kzg_ctx* ctx, uint32_t i, const uint8_t* row_be32, uint64_t T, int evaluation_form,
             const uint8_t alpha_be32[32], uint8_t out_eval32[32], uint8_t out_proof48[48]) {
    if (!out_proof48) return KZG_E_ARG;
    return commit_open_host(ctx, i, row_be32, T, evaluation_form, alpha_be32, nullptr, out_eval32, out_proof48);
}
int kzg_commit_open(kzg_ctx* ctx, uint32_t i, const uint8_t* row_be32, uint64_t T, int evaluation_form,
                    const uint8_t alpha_be32[32], uint8_t out_commitment48[48], uint8_t out_eval32[32],
                    uint8_t out_proof48[48]) {
    if (!out_commitment48 || !out_proof48) return KZG_E_ARG;
    return commit_open_host(ctx, i, row_be32, T, evaluation_form, alpha_be32, out_commitment48, out_eval32,
                            out_proof48);
}

// 32 big-endian bytes < r (host check of the batched opening's alpha and gamma: an argument error, not a queued failure)
static bool fr_be32_canonical(const uint8_t b[32]) {
    static const uint8_t R_BE[32] = {0x73, 0xED, 0xA7, 0x53, 0x29, 0x9D, 0x7D, 0x48, 0x33, 0x39, 0xD8, 0x08, 0x09, 0xA1, 0xD8, 0x05,
                                     0x53, 0xBD, 0xA4, 0x02, 0xFF, 0xFE, 0x5B, 0xFE, 0xFF, 0xFF, 0xFF, 0xFF, 0x00, 0x00, 0x00, 0x01};
    return memcmp(b, R_BE, 32) < 0;
}
// k rows of worker i opened at one point with ONE proof for sum_j gamma^j f_j (pipeline.hip: commit_open_batch_dev)
int kzg_commit_open_batch(kzg_ctx* ctx, uint32_t i, uint32_t k, const uint8_t* rows_be32, uint64_t T, int evaluation_form,
                          const uint8_t alpha_be32[32], const uint8_t gamma_be32[32], uint8_t* out_commitments48,
                          uint8_t* out_evals32, uint8_t out_proof48[48]) {
    if (!ctx || !rows_be32 || !alpha_be32 || !gamma_be32 || !out_commitments48 || !out_evals32 || !out_proof48)
        return KZG_E_ARG;
    if (k == 0 || k > KZG_MAX_BATCH_OPEN) return fail(ctx, KZG_E_ARG, "batched opening: k must be in [1, KZG_MAX_BATCH_OPEN]");
    if (!fr_be32_canonical(alpha_be32) || !fr_be32_canonical(gamma_be32))
        return fail(ctx, KZG_E_ARG, "batched opening: alpha and gamma must be canonical scalars (< r)");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    LaneHold H(ctx);
    if (int rc = H.take()) return rc;
    Lane& L = H.L();
    int rc = check_worker(ctx, i, T);
    if (rc) return rc;
    if (evaluation_form && T > 1 && ilog2_exact(T) < 0)
        return fail(ctx, KZG_E_ARG, "evaluation-form row length must be a power of two");
    prof_begin(ctx, L);
    rc = clear_flags(ctx, L);
    if (rc) return rc;
    HIPCHK(ctx, L.coeffA.ensure(k * T * 32));
    rc = upload_fr(ctx, L, rows_be32, k * T, L.coeffA.as<uint32_t>(), 1);
    if (rc) return rc;
    return commit_open_batch_dev(ctx, H, i, L.coeffA.as<uint32_t>(), k, T, evaluation_form, alpha_be32, gamma_be32,
                                 out_commitments48, out_evals32, out_proof48);
}

// k rows of worker i opened at m points, one proof per point (pipeline.hip: commit_open_multi_dev)
int kzg_commit_open_multi(kzg_ctx* ctx, uint32_t i, uint32_t k, const uint8_t* rows_be32, uint64_t T, int evaluation_form,
                          uint32_t m, const uint8_t* points_be32, const uint32_t* masks, const uint8_t* gammas_be32,
                          uint8_t* out_commitments48, uint8_t* out_evals32, uint8_t* out_proofs48) {
    if (!ctx || !rows_be32 || !points_be32 || !masks || !gammas_be32 || !out_commitments48 || !out_evals32 || !out_proofs48)
        return KZG_E_ARG;
    if (k == 0 || k > KZG_MAX_BATCH_OPEN) return fail(ctx, KZG_E_ARG, "multi-point opening: k must be in [1, KZG_MAX_BATCH_OPEN]");
    if (m == 0 || m > KZG_MAX_OPEN_POINTS)
        return fail(ctx, KZG_E_ARG, "multi-point opening: m must be in [1, KZG_MAX_OPEN_POINTS]");
    for (uint32_t p = 0; p < m; p++) {
        if (masks[p] == 0 || (masks[p] >> k) != 0)
            return fail(ctx, KZG_E_ARG, "multi-point opening: every mask must name at least one row, and rows < k only");
        if (!fr_be32_canonical(points_be32 + 32 * (size_t)p) || !fr_be32_canonical(gammas_be32 + 32 * (size_t)p))
            return fail(ctx, KZG_E_ARG, "multi-point opening: points and gammas must be canonical scalars (< r)");
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    LaneHold H(ctx);
    if (int rc = H.take()) return rc;
    Lane& L = H.L();
    int rc = check_worker(ctx, i, T);
    if (rc) return rc;
    if (evaluation_form && T > 1 && ilog2_exact(T) < 0)
        return fail(ctx, KZG_E_ARG, "evaluation-form row length must be a power of two");
    prof_begin(ctx, L);
    rc = clear_flags(ctx, L);
    if (rc) return rc;
    HIPCHK(ctx, L.coeffA.ensure(k * T * 32));
    rc = upload_fr(ctx, L, rows_be32, k * T, L.coeffA.as<uint32_t>(), 1);
    if (rc) return rc;
    return commit_open_multi_dev(ctx, H, i, L.coeffA.as<uint32_t>(), k, T, evaluation_form, m, points_be32, masks,
                                 gammas_be32, out_commitments48, out_evals32, out_proofs48);
}

static int ntt_dev(kzg_ctx* ctx, Lane& L, uint32_t* data, uint64_t n, int inverse) {  // in place via coeffB
    int lg = ilog2_exact(n);
    if (lg < 0) return fail(ctx, KZG_E_ARG, "NTT length must be a power of two");
    uint32_t *tw = nullptr, *invn = nullptr;
    int rc = ensure_twiddles(ctx, L, lg, inverse, &tw, inverse ? &invn : nullptr);
    if (rc) return rc;
    HIPCHK(ctx, L.coeffB.ensure(n * 32));
    HIPCHK(ctx, L.ntt_mid.ensure(n * 48));
    {
        Span sp(ctx, L, KZG_T_NTT);
        launch_fr_ntt(L.stream, data, L.coeffB.as<uint32_t>(), lg, tw, inverse ? invn : nullptr, L.ntt_mid.as<uint32_t>());
        HIPCHK(ctx, hipMemcpyAsync(data, L.coeffB.p, n * 32, hipMemcpyDeviceToDevice, L.stream));
    }
    return KZG_OK;
}
int kzg_ntt(kzg_ctx* ctx, uint8_t* inout_be32, uint64_t n, int inverse) {
    if (!ctx || !inout_be32 || !n) return KZG_E_ARG;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    LaneHold H(ctx);
    if (int rc = H.take()) return rc;
    Lane& L = H.L();
    prof_begin(ctx, L);
    int rc = clear_flags(ctx, L);
    if (rc) return rc;
    HIPCHK(ctx, L.coeffA.ensure(n * 32));
    HIPCHK(ctx, L.out_be.ensure(n * 32));
    rc = upload_fr(ctx, L, inout_be32, n, L.coeffA.as<uint32_t>(), 1);
    if (rc) return rc;
    rc = ntt_dev(ctx, L, L.coeffA.as<uint32_t>(), n, inverse);
    if (rc) return rc;
    launch_fr_to_be(L.stream, L.coeffA.as<uint32_t>(), L.out_be.as<uint8_t>(), n, 1);
    rc = finish(ctx, L);
    if (rc) return rc;
    HIPCHK(ctx, hipMemcpy(inout_be32, L.out_be.p, n * 32, hipMemcpyDeviceToHost));
    H.clean = true;
    return KZG_OK;
}
int kzg_eval(kzg_ctx* ctx, const uint8_t* coeffs_be32, uint64_t n, const uint8_t x_be32[32], uint8_t out_be32[32]) {
    if (!ctx || !x_be32 || !out_be32 || (n && !coeffs_be32)) return KZG_E_ARG;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (n == 0) {
        memset(out_be32, 0, 32);
        return KZG_OK;
    }
    LaneHold H(ctx);
    if (int rc = H.take()) return rc;
    Lane& L = H.L();
    prof_begin(ctx, L);
    int rc = clear_flags(ctx, L);
    if (rc) return rc;
    HIPCHK(ctx, L.coeffA.ensure(n * 32));
    HIPCHK(ctx, L.hbuf.ensure(poly_level_words(n) * 4));
    HIPCHK(ctx, L.hnext.ensure(poly_level_words(n) * 4));
    rc = upload_fr(ctx, L, coeffs_be32, n, L.coeffA.as<uint32_t>(), 1);
    if (rc) return rc;
    uint32_t* x_m = reinterpret_cast<uint32_t*>(L.tail + TB_ALPHA_M);
    uint32_t* y_m = reinterpret_cast<uint32_t*>(L.tail + TB_Y_M);
    launch_poly_open(L.stream, L.coeffA.as<uint32_t>(), n, x_m, L.hbuf.as<uint32_t>(), L.hnext.as<uint32_t>(), y_m, nullptr,
                     x_be32, L.flags(), L.tail + TB_EVAL);
    rc = finish(ctx, L);
    if (rc) return rc;
    memcpy(out_be32, L.pin + TB_EVAL, 32);
    H.clean = true;
    return KZG_OK;
}

// y = (NTT or inverse NTT of vals)(x): the validator's per-row challenge step -- fft(poly[i], left=True, inverse=True) then
// eval(coefficients, alpha) (reference neurons/validator.py:115-118) -- without the round trip of 2^16 coefficients through
// text between the two
int kzg_ntt_eval(kzg_ctx* ctx, const uint8_t* vals_be32, uint64_t n, int inverse, const uint8_t x_be32[32],
                 uint8_t out_y32[32]) {
    if (!ctx || !vals_be32 || !n || !x_be32 || !out_y32) return KZG_E_ARG;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int lg = ilog2_exact(n);
    if (lg < 0) return fail(ctx, KZG_E_ARG, "NTT length must be a power of two");
    LaneHold H(ctx);
    if (int rc = H.take()) return rc;
    Lane& L = H.L();
    prof_begin(ctx, L);
    int rc = clear_flags(ctx, L);
    if (rc) return rc;
    HIPCHK(ctx, L.coeffA.ensure(n * 32));
    HIPCHK(ctx, L.coeffB.ensure(n * 32));
    HIPCHK(ctx, L.ntt_mid.ensure(n * 48));
    HIPCHK(ctx, L.hbuf.ensure(poly_level_words(n) * 4));
    HIPCHK(ctx, L.hnext.ensure(poly_level_words(n) * 4));
    rc = upload_fr(ctx, L, vals_be32, n, L.coeffA.as<uint32_t>(), 1);
    if (rc) return rc;
    const uint32_t* coeffs = L.coeffA.as<uint32_t>();
    if (lg > 0) {
        uint32_t *tw = nullptr, *invn = nullptr;
        rc = ensure_twiddles(ctx, L, lg, inverse, &tw, inverse ? &invn : nullptr);
        if (rc) return rc;
        Span sp(ctx, L, KZG_T_NTT);
        launch_fr_ntt(L.stream, L.coeffA.as<uint32_t>(), L.coeffB.as<uint32_t>(), lg, tw, inverse ? invn : nullptr,
                      L.ntt_mid.as<uint32_t>());
        coeffs = L.coeffB.as<uint32_t>();
    }
    uint32_t* x_m = reinterpret_cast<uint32_t*>(L.tail + TB_ALPHA_M);
    uint32_t* y_m = reinterpret_cast<uint32_t*>(L.tail + TB_Y_M);
    launch_poly_open(L.stream, coeffs, n, x_m, L.hbuf.as<uint32_t>(), L.hnext.as<uint32_t>(), y_m, nullptr, x_be32, L.flags(),
                     L.tail + TB_EVAL);
    rc = finish(ctx, L);
    if (rc) return rc;
    memcpy(out_y32, L.pin + TB_EVAL, 32);
    H.clean = true;
    return KZG_OK;
}

int kzg_upload_fr(kzg_ctx* ctx, int slot, const uint8_t* be32, uint64_t n, int to_mont) {
    if (!ctx || slot < 0 || slot >= N_SLOTS || (n && !be32)) return KZG_E_ARG;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    LaneHold H(ctx);
    if (int rc = H.take_all()) return rc;   // no request may be reading the slot
    Lane& L = H.L();
    prof_begin(ctx, L);
    int rc = clear_flags(ctx, L);
    if (rc) return rc;
    ctx->slot_n[slot] = 0;
    HIPCHK(ctx, ctx->slot[slot].ensure(n * 32 + 32));
    rc = upload_fr(ctx, L, be32, n, ctx->slot[slot].as<uint32_t>(), to_mont);
    if (rc) return rc;
    rc = finish(ctx, L);
    if (rc) return rc;
    ctx->slot_n[slot] = n;
    ctx->slot_mont[slot] = to_mont ? 1 : 0;
    H.clean = true;
    return KZG_OK;
}
// dev_out != null: the 192-byte partial is left in the CALLER's device buffer (e.g. a torch tensor about to enter an
// RCCL all_gather) instead of coming back to the host
static int msm_resident_common(kzg_ctx* ctx, int slot, uint64_t n, uint64_t srs_offset, uint8_t* out, bool partial,
                               void* dev_out = nullptr) {
    if (!ctx || (!out && !dev_out) || slot < 0 || slot >= N_SLOTS) return KZG_E_ARG;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    LaneHold H(ctx);
    if (int rc = H.take()) return rc;
    Lane& L = H.L();
    int rc = need_srs(ctx);
    if (rc) return rc;
    if (n > ctx->slot_n[slot]) return fail(ctx, KZG_E_ARG, "slot holds fewer scalars than requested");
    prof_begin(ctx, L);
    rc = clear_flags(ctx, L);
    if (rc) return rc;
    rc = msm_core(ctx, L, ScalarSets::one(ctx->slot[slot].as<uint32_t>(), ctx->slot_mont[slot]), n, srs_offset, L.res());
    if (rc) return rc;
    if (dev_out) launch_xyzz_pack(L.stream, L.res(), reinterpret_cast<uint32_t*>(dev_out), 1);
    else if (partial) queue_pack(ctx, L);
    else queue_encode(ctx, L, true, false);
    rc = finish(ctx, L);  // synchronises the stream: dev_out is complete when the call returns
    if (rc) return rc;
    if (out) {
        if (partial) result_partial(ctx, L, out);
        else result_c48(ctx, L, 0, out);
    }
    H.clean = true;
    return KZG_OK;
}
int kzg_msm_partial_resident_dev(kzg_ctx* ctx, int slot, uint64_t n, uint64_t srs_offset, void* dev_out_xyzz192) {
    if (!dev_out_xyzz192) return KZG_E_ARG;
    return msm_resident_common(ctx, slot, n, srs_offset, nullptr, true, dev_out_xyzz192);
}
int kzg_msm_resident(kzg_ctx* ctx, int slot, uint64_t n, uint64_t srs_offset, uint8_t out48[48]) {
    return msm_resident_common(ctx, slot, n, srs_offset, out48, false);
}
int kzg_msm_partial_resident(kzg_ctx* ctx, int slot, uint64_t n, uint64_t srs_offset, uint8_t out_xyzz192[192]) {
    return msm_resident_common(ctx, slot, n, srs_offset, out_xyzz192, true);
}
// ---- ticketed MSM: submit returns once the work is queued on a free lane, wait returns the result, so MSM i+1 (sort,
// accumulate) overlaps the latency-bound tail (fold, bucket tree, final combination) of MSM i from ONE host thread.
// (Several host threads get the same overlap from the blocking calls: each call runs on its own lane.)
int kzg_msm_submit(kzg_ctx* ctx, int slot, uint64_t n, uint64_t srs_offset, int partial, int* out_ticket) {
    if (!ctx || !out_ticket || slot < 0 || slot >= N_SLOTS) return KZG_E_ARG;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int li = -1;
    int rc = lane_acquire(ctx, LANE_TICKET, &li);
    if (rc) return rc;
    Lane& L = ctx->lane[li];
    // checked while the lane is held: an exclusive operation (SRS reload, kzg_upload_fr) cannot slip in between
    rc = need_srs(ctx);
    if (!rc && n > ctx->slot_n[slot]) rc = fail(ctx, KZG_E_ARG, "slot holds fewer scalars than requested");
    if (rc) {
        lane_release(ctx, li);
        return rc;
    }
    prof_begin(ctx, L);
    rc = clear_flags(ctx, L);
    if (!rc) rc = msm_core(ctx, L, ScalarSets::one(ctx->slot[slot].as<uint32_t>(), ctx->slot_mont[slot]), n, srs_offset, L.res());
    if (!rc) {
        L.partial = partial != 0;
        if (partial) queue_pack(ctx, L);
        else queue_encode(ctx, L, true, false);
        prof_close(ctx, L);
        launch_publish(L.stream, L.tail, L.pin_dev, TB_COPY, L.flags(), reinterpret_cast<uint32_t*>(L.pin_dev + PIN_SEQ),
                       ++L.pub_seq);
        hipError_t e = hipEventRecord(L.ev_done, L.stream);
        if (e == hipSuccess) e = hipGetLastError();
        if (e != hipSuccess) rc = fail(ctx, KZG_E_HIP, std::string("kzg_msm_submit: ") + hipGetErrorString(e));
    }
    if (rc) {  // nothing may still be running on the lane's buffers when it becomes reusable
        L.sort_ws_clean = false;
        (void)hipStreamSynchronize(L.stream);
        (void)hipGetLastError();
        lane_release(ctx, li);
        return rc;
    }
    *out_ticket = li;
    return KZG_OK;
}
int kzg_msm_wait(kzg_ctx* ctx, int ticket, uint8_t* out) {
    if (!ctx || !out || ticket < 0 || ticket >= N_LANES) return KZG_E_ARG;
    Lane& L = ctx->lane[ticket];
    if (int rc0 = ticket_claim(ctx, ticket)) return rc0;   // exactly one waiter per ticket
    (void)hipSetDevice(ctx->device);
    hipError_t e = hipSuccess;  // not under the lock: other threads submit / run meanwhile
#ifndef KZG_NO_POLL
    if (ctx->profiling == 1 || !L.expect_short || !poll_pinned(ctx, L, PIN_SEQ, L.pub_seq))
#endif
        e = hipEventSynchronize(L.ev_done);
    int rc = KZG_OK;
    if (e != hipSuccess) {
        rc = fail(ctx, KZG_E_HIP, std::string("hipEventSynchronize(ticket): ") + hipGetErrorString(e));
        (void)hipStreamSynchronize(L.stream);
    } else {
        L.flags_clean = true;
        prof_end(ctx, L);
        if (L.partial) result_partial(ctx, L, out);
        else result_c48(ctx, L, 0, out);
    }
    lane_release(ctx, ticket);
    return rc;
}

// gives up an outstanding ticket (kzg_msm_submit / kzg_msm_sharded_begin) whose result will never be collected -- e.g. the
// collective between _begin and _finish raised: drains the lane and frees it
int kzg_msm_cancel(kzg_ctx* ctx, int ticket) {
    if (!ctx || ticket < 0 || ticket >= N_LANES) return KZG_E_ARG;
    Lane& L = ctx->lane[ticket];
    if (int rc0 = ticket_claim(ctx, ticket)) return rc0;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(L.stream);
    (void)hipGetLastError();
    L.spans.clear();
    L.flags_clean = false;     // its publish may not have run: the next request clears the flag words itself
    L.sort_ws_clean = false;
    lane_release(ctx, ticket);
    return KZG_OK;
}

int kzg_commit_open_resident(kzg_ctx* ctx, uint32_t i, int slot, uint64_t T, int evaluation_form,
                             const uint8_t alpha_be32[32], uint8_t out_commitment48[48], uint8_t out_eval32[32],
                             uint8_t out_proof48[48]) {
    if (!ctx || slot < 0 || slot >= N_SLOTS || !alpha_be32 || !out_commitment48 || !out_eval32 || !out_proof48)
        return KZG_E_ARG;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    LaneHold H(ctx);
    if (int rc = H.take()) return rc;
    Lane& L = H.L();
    int rc = check_worker(ctx, i, T);
    if (rc) return rc;
    if (T > ctx->slot_n[slot] || !ctx->slot_mont[slot])
        return fail(ctx, KZG_E_ARG, "slot must hold >= T Montgomery-form elements (kzg_upload_fr(.., to_mont=1))");
    prof_begin(ctx, L);
    rc = clear_flags(ctx, L);
    if (rc) return rc;
    return commit_open_dev(ctx, H, i, ctx->slot[slot].as<uint32_t>(), T, evaluation_form, alpha_be32, out_commitment48,
                           out_eval32, out_proof48);
}
int kzg_ntt_resident(kzg_ctx* ctx, int slot, uint64_t n, int inverse) {
    if (!ctx || slot < 0 || slot >= N_SLOTS || !n) return KZG_E_ARG;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    LaneHold H(ctx);
    if (int rc = H.take_all()) return rc;   // rewrites the slot in place
    Lane& L = H.L();
    if (n > ctx->slot_n[slot] || !ctx->slot_mont[slot]) return fail(ctx, KZG_E_ARG, "slot must hold >= n Montgomery elements");
    prof_begin(ctx, L);
    int rc = clear_flags(ctx, L);
    if (rc) return rc;
    rc = ntt_dev(ctx, L, ctx->slot[slot].as<uint32_t>(), n, inverse);
    if (rc) return rc;
    rc = finish(ctx, L);
    if (rc) return rc;
    H.clean = true;
    return KZG_OK;
}

// The rate that bounds the accumulate kernel, measured now, on this device (csrc/calibrate.hip).  Exclusive: waits for
// the lanes to be idle so that nothing shares the SIMDs with the measurement.
int kzg_calibrate(kzg_ctx* ctx, int waves_per_simd, double out[6]) {
    if (!ctx || !out) return KZG_E_ARG;
    if (waves_per_simd < 1 || waves_per_simd > 8) return fail(ctx, KZG_E_ARG, "waves_per_simd must be in [1, 8]");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipDeviceProp_t prop;
    HIPCHK(ctx, hipGetDeviceProperties(&prop, ctx->device));
    const uint32_t cus = (uint32_t)prop.multiProcessorCount, simds = 4 * cus;
    LaneHold H(ctx);
    if (int rc = H.take_all()) return rc;
    Lane& L = H.L();
    const uint32_t blocks = cus * (uint32_t)waves_per_simd;      // 256 threads = 4 waves = one per SIMD of a CU
    HIPCHK(ctx, L.out_be.ensure((2 + (size_t)blocks * 256) * sizeof(uint64_t)));
    uint64_t* d = L.out_be.as<uint64_t>();
    hipEvent_t e0 = nullptr, e1 = nullptr;
    HIPCHK(ctx, hipEventCreate(&e0));
    if (hipEventCreate(&e1) != hipSuccess) { (void)hipEventDestroy(e0); return fail(ctx, KZG_E_HIP, "hipEventCreate"); }
    // ~1.5 ms at 2 waves per SIMD (2.3 ns per wave-instruction per SIMD); a short launch first pages the code in
    const uint32_t iters = 40960u * 2u / (uint32_t)std::max(2, waves_per_simd);
    launch_calibrate_mad(L.stream, d, blocks, iters / 16);
    (void)hipEventRecord(e0, L.stream);
    launch_calibrate_mad(L.stream, d, blocks, iters);
    (void)hipEventRecord(e1, L.stream);
    uint64_t ticks = 0;
    hipError_t err = hipMemcpyAsync(&ticks, d, sizeof(ticks), hipMemcpyDeviceToHost, L.stream);
    if (err == hipSuccess) err = hipStreamSynchronize(L.stream);
    float ms = 0;
    if (err == hipSuccess) err = hipEventElapsedTime(&ms, e0, e1);
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    if (err != hipSuccess) return fail(ctx, KZG_E_HIP, std::string("kzg_calibrate: ") + hipGetErrorString(err));
    const double inst_per_wave = (double)iters * calibrate_unroll();
    const double inst_per_simd = inst_per_wave * waves_per_simd;
    out[0] = (double)ms * 1e6 / inst_per_simd;                   // ns per v_mad_u64_u32 wave-instruction per SIMD
    out[1] = (double)simds / out[0];                             // G wave-mads per second, whole chip
    out[2] = ms > 0 ? (double)ticks / ((double)ms * 1e6) : 0;    // s_memtime ticks per ns over the launch (wave 0)
    out[3] = (double)ms;
    out[4] = (double)simds;
    out[5] = (double)ticks / inst_per_wave;                      // ticks per instruction of ONE wave
    H.clean = true;
    return KZG_OK;
}

}  // extern "C"

// ---- committed row sets (kzg_rows_*): the set table of kzg_ctx (ctx.hip.h) around the two halves of the multi-point
// opening (pipeline.hip: rows_commit_dev, rows_open_dev).  Lock order: a lane first, then sets_mu (an SRS load holds every
// lane when it marks the sets stale, so no open or commit runs across it).
namespace kzg_impl {

static std::atomic<uint64_t> g_row_set_handles{0};   // never reused within the process: a stale handle names no newer set

static uint32_t rows_live(const kzg_ctx* ctx) {   // under sets_mu
    uint32_t n = 0;
    for (const auto& kv : ctx->sets) n += !kv.second.released;
    return n;
}
// retire a set (under sets_mu): its buffer goes to the free list -- no hipFree while other lanes run
static void rows_retire(kzg_ctx* ctx, std::map<uint64_t, kzg_ctx::RowSet>::iterator it) {
    if (it->second.buf.p) ctx->sets_free.push_back(std::move(it->second.buf));
    ctx->sets.erase(it);
}
void rows_invalidate(kzg_ctx* ctx) {
    std::lock_guard<std::mutex> lk(ctx->sets_mu);
    for (auto& kv : ctx->sets) {   // every lane is held: no open reads these buffers
        kv.second.stale = true;
        kv.second.buf.release();
    }
    ctx->sets_free.clear();
}
// a commit's reservation against KZG_MAX_ROW_SETS and its buffer until the set is inserted.  Declared before the call's
// LaneHold, so that a failed call has drained its lane before the buffer goes back to the free list.
struct RowsPending {
    kzg_ctx* ctx;
    DevBuf buf;
    bool reserved = false;
    ~RowsPending() {
        std::lock_guard<std::mutex> lk(ctx->sets_mu);
        if (reserved) ctx->sets_pending--;
        if (buf.p) ctx->sets_free.push_back(std::move(buf));
    }
};
// a new set's place under KZG_MAX_ROW_SETS and its buffer of `bytes` bytes (lane held): the smallest released buffer that
// fits, else a fresh allocation.  KZG_E_BUSY when the sets are all taken, KZG_E_NOMEM when the device has no room.
static int rows_reserve(kzg_ctx* ctx, const char* what, RowsPending& pend, size_t bytes) {
    {
        std::lock_guard<std::mutex> lk(ctx->sets_mu);
        if (rows_live(ctx) + ctx->sets_pending >= KZG_MAX_ROW_SETS)
            return fail(ctx, KZG_E_BUSY, std::string(what) + ": KZG_MAX_ROW_SETS sets are live: release one first");
        ctx->sets_pending++;
        pend.reserved = true;
        size_t best = ctx->sets_free.size();
        for (size_t b = 0; b < ctx->sets_free.size(); b++)
            if (ctx->sets_free[b].cap >= bytes && (best == ctx->sets_free.size() || ctx->sets_free[b].cap < ctx->sets_free[best].cap))
                best = b;
        if (best < ctx->sets_free.size()) {
            pend.buf = std::move(ctx->sets_free[best]);
            ctx->sets_free.erase(ctx->sets_free.begin() + best);
        }
    }
    HIPCHK(ctx, pend.buf.ensure(bytes));
    return KZG_OK;
}
// the reserved set becomes live: k rows of T coefficients of worker i in pend's buffer; returns its handle
static uint64_t rows_insert(kzg_ctx* ctx, RowsPending& pend, uint32_t i, uint32_t k, uint64_t T) {
    const uint64_t h = ++g_row_set_handles;
    std::lock_guard<std::mutex> lk(ctx->sets_mu);
    kzg_ctx::RowSet& st = ctx->sets[h];
    st.i = i;
    st.k = k;
    st.T = T;
    st.buf = std::move(pend.buf);
    ctx->sets_pending--;
    pend.reserved = false;
    return h;
}
// the references an open holds on its sets, dropped after its lane is drained (declared before the LaneHold)
struct RowsRefs {
    kzg_ctx* ctx;
    uint64_t h[KZG_MAX_BATCH_OPEN];
    uint32_t n = 0;
    ~RowsRefs() {
        std::lock_guard<std::mutex> lk(ctx->sets_mu);
        for (uint32_t t = 0; t < n; t++) {
            auto it = ctx->sets.find(h[t]);
            if (it != ctx->sets.end() && --it->second.refs == 0 && it->second.released) rows_retire(ctx, it);
        }
    }
};

// the sets named by `handles` (lane held, so that an SRS load cannot free their buffers under the caller): their rows into
// rt, numbered by concatenation, the worker and row length into *i / *T, one reference per set into refs.  `what` prefixes
// the messages.
static int rows_lookup(kzg_ctx* ctx, const char* what, uint32_t expect_i, uint32_t n_handles, const uint64_t* handles,
                       RowsRefs& refs, RowTab& rt, uint32_t* out_k, uint32_t* out_i, uint64_t* out_T) {
    auto bad = [&](const char* why) { return fail(ctx, KZG_E_ARG, std::string(what) + why); };
    memset(&rt, 0, sizeof(rt));
    uint32_t k = 0, i = 0;
    uint64_t T = 0;
    std::lock_guard<std::mutex> lk(ctx->sets_mu);
    for (uint32_t t = 0; t < n_handles; t++) {
        auto it = ctx->sets.find(handles[t]);
        if (it == ctx->sets.end() || it->second.released) return bad(": unknown or released handle");
        kzg_ctx::RowSet& st = it->second;
        if (st.acc) return bad(": the handle names a quotient accumulator, not a row set");
        if (st.stale)
            return bad(": the set was committed under an SRS that has since been reloaded (its commitments no longer "
                       "hold): release it and commit its rows again");
        if (t == 0) {
            i = st.i;
            T = st.T;
        } else if (st.i != i || st.T != T) {
            return bad(": all sets must belong to one worker and have one row length");
        }
        if (expect_i != UINT32_MAX && st.i != expect_i) return bad(": the set belongs to another worker");
        if (k + st.k > KZG_MAX_BATCH_OPEN) return bad(": more than KZG_MAX_BATCH_OPEN rows in all");
        for (uint32_t j = 0; j < st.k; j++) rt.r[k + j] = st.buf.as<uint32_t>() + (uint64_t)j * st.T * 8;
        k += st.k;
        st.refs++;
        refs.h[refs.n++] = handles[t];
    }
    *out_k = k;
    *out_i = i;
    *out_T = T;
    return KZG_OK;
}

// ---- the call frame of the column builders (sorted, derived, int, alu, wide, poseidon, expr, recurrence, fetch): a set
// built FROM sets, whose columns may carry the caller's tail behind row `usable`.

// What differs between the builders' `usable` / `tail_be32` layouts: what usable = 0 means, in the words of the first refusal,
// and whether row `usable` closes a running value (recurrence), so that a column takes T - usable - 1 tail scalars, not T - usable
struct LayoutKind {
    const char* zero_means;
    uint32_t closing;
};
static const LayoutKind LAY_READ = {"all T rows are read", 0}, LAY_SORTED = {"all T rows are sorted", 0},
                        LAY_EVALUATED = {"all T rows are evaluated", 0}, LAY_CLOSING = {"the plain layout", 1};
// the layout `lay` as the caller gave it against the row length, over n_cols committed columns.  The tail may be null when it
// holds no scalar (nothing is committed, or usable = T - 1 before a closing row).  *out: what to pass down, null for usable = 0
static int layout_check(kzg_ctx* ctx, const char* what, const Blind& lay, uint64_t T, uint32_t n_cols, const LayoutKind& kind,
                        const Blind** out) {
    auto bad = [&](const std::string& why) { return fail(ctx, KZG_E_ARG, std::string(what) + why); };
    *out = lay.usable ? &lay : nullptr;
    if (!lay.usable) return lay.tail_be32 ? bad(": tail_be32 must be null in the plain layout (usable = 0)") : KZG_OK;
    if (lay.usable >= T) return bad(std::string(": usable must be in [1, T - 1] (0: ") + kind.zero_means + ")");
    if (T - lay.usable > KZG_MAX_BLIND_ROWS) return bad(": at most KZG_MAX_BLIND_ROWS rows may lie at or behind row `usable`");
    const uint64_t n_tail = (uint64_t)n_cols * (T - lay.usable - kind.closing);
    if (n_tail && !lay.tail_be32)
        return bad(kind.closing ? ": tail_be32 may be null only when usable = T - 1" : ": tail_be32 must be given when usable > 0");
    for (uint64_t j = 0; j < n_tail; j++)
        if (!fr_be32_canonical(lay.tail_be32 + 32 * (size_t)j)) return bad(": tail scalars must be canonical (< r)");
    return KZG_OK;
}

// One call of a column builder: begin() -- the builder's checks on row indices -- ready() -- the device call -- commit().
struct BuilderCall {
    kzg_ctx* ctx;
    const char* what;       // prefixes the messages
    // The order of these three is load-bearing: members are destroyed in reverse, so the LaneHold drains the lane of a failed
    // call BEFORE the references are dropped and the reserved buffer returns to the free list -- kernels may still write it.
    RowsPending pend;
    RowsRefs refs[3];       // one per handle list
    LaneHold H;
    uint32_t n_lists = 0, i = 0, n_out = 0;
    uint64_t T = 0;
    Blind lay = {0, nullptr};
    const Blind* blind = nullptr;   // the layout to pass down, set by ready()
    BuilderCall(kzg_ctx* c, const char* w) : ctx(c), what(w), pend{c}, refs{{c}, {c}, {c}}, H(c) {}
    // a further handle list (`list` prefixes its messages): its rows into rt, their number into *k; every list of the call
    // must be of one worker and one row length
    int lookup(const char* list, uint32_t expect_i, uint32_t n_handles, const uint64_t* handles, RowTab& rt, uint32_t* k) {
        uint32_t i2 = 0;
        uint64_t T2 = 0;
        if (int rc = rows_lookup(ctx, list, expect_i, n_handles, handles, refs[n_lists], rt, k, &i2, &T2)) return rc;
        if (n_lists++ == 0) {
            i = i2;
            T = T2;
        } else if (i2 != i || T2 != T) {
            return fail(ctx, KZG_E_ARG, std::string(what) + ": all sets must belong to one worker and have one row length");
        }
        return KZG_OK;
    }
    // the device, the lane (before the lookups: an SRS load cannot free the sets' buffers under this call), the first list
    int begin(const char* list, uint32_t expect_i, uint32_t n_handles, const uint64_t* handles, RowTab& rt, uint32_t* k) {
        HIPCHK(ctx, hipSetDevice(ctx->device));
        if (int rc = H.take()) return rc;
        return lookup(list, expect_i, n_handles, handles, rt, k);
    }
    // the worker, the row length (a power of two, at most 2^max_log_t where the builder has a cap: 0 for none), the layout
    // `asked` over the n_cols columns to commit, their reservation (none for n_cols = 0), then the call's profile and flags
    int ready(uint32_t n_cols, int max_log_t, const Blind& asked, const LayoutKind& kind) {
        if (int rc = check_worker(ctx, i, T)) return rc;
        if (ilog2_exact(T) < 0) return fail(ctx, KZG_E_ARG, std::string(what) + ": the row length must be a power of two");
        if (max_log_t && T > ((uint64_t)1 << max_log_t))
            return fail(ctx, KZG_E_ARG, std::string(what) + ": the row length must be at most 2^" + std::to_string(max_log_t));
        lay = asked;
        n_out = n_cols;
        if (int rc = layout_check(ctx, what, lay, T, n_cols, kind, &blind)) return rc;
        if (n_out)
            if (int rc = rows_reserve(ctx, what, pend, (size_t)n_out * T * 32)) return rc;
        prof_begin(ctx, H.L());
        return clear_flags(ctx, H.L());
    }
    uint32_t* dst() { return n_out ? pend.buf.as<uint32_t>() : nullptr; }   // the new set's buffer
    uint64_t commit() { return n_out ? rows_insert(ctx, pend, i, n_out, T) : 0; }   // the new set's handle; 0: nothing committed
};

// ---- the unit builders (rows_poseidon .. rows_edwards): a call is 1 .. N units, each with a mode, slots that are a row index
// or an immediate, an out / cols list and an optional expect that makes it a check; what they share around their unit loops.

// The distinct rows the units of a call name, and the largest.  A call may read at most KZG_MAX_BATCH_OPEN distinct rows, so
// one more than that is all that is ever held: past the capacity a new row is counted, not stored, and max_row goes on.
struct SeenRows {
    static constexpr uint32_t CAP = KZG_MAX_BATCH_OPEN + 1;
    uint32_t n = 0, max_row = 0, rows[CAP];
    void see(uint32_t row) {
        max_row = std::max(max_row, row);
        const uint32_t held = std::min(n, CAP);
        uint32_t d = 0;
        while (d < held && rows[d] != row) d++;
        if (d < held) return;
        if (n < CAP) rows[n] = row;
        n++;
    }
    // the `count` rows from `first` (a wide value of ec); a row at or beyond 2^32 - 1 ends the run and fails the index check
    void see_run(uint32_t first, uint32_t count) {
        for (uint32_t l = 0; l < count; l++) {
            const uint64_t row = (uint64_t)first + l;   // (cannot wrap a uint64)
            if (row >= 0xffffffffull) {
                max_row = 0xffffffffu;
                return;
            }
            see((uint32_t)row);
        }
    }
    bool too_many() const { return n > KZG_MAX_BATCH_OPEN; }
};

// One call of a unit builder: handles_ok() -- the builder's checks -- open() -- the device call, the statistics -- finish().
// (Constructed behind the host's checks: a refused call touches no context.)
struct UnitCall : BuilderCall {
    RowTab it;                                // the input rows
    uint8_t c48[KZG_MAX_BATCH_OPEN * 48];     // the commitments, until the call can no longer fail
    using BuilderCall::BuilderCall;
    static int handles_ok(kzg_ctx* ctx, const char* what, uint32_t n_handles) {
        if (n_handles == 0 || n_handles > KZG_MAX_BATCH_OPEN)
            return fail(ctx, KZG_E_ARG, std::string(what) + ": the number of handles must be in [1, KZG_MAX_BATCH_OPEN]");
        return KZG_OK;
    }
    // begin; the refusal of a row beyond the input rows, in the builder's words (rows_named: whether the call names any); ready
    // over the n_cols columns to commit in the column builders' layout
    int open(uint32_t expect_i, uint32_t n_handles, const uint64_t* handles, bool rows_named, uint32_t max_row, const char* row_why,
             uint32_t n_cols, const kzg_derive_opts* opts) {
        uint32_t ki = 0;
        if (int rc = begin(what, expect_i, n_handles, handles, it, &ki)) return rc;
        if (rows_named && max_row >= ki) return fail(ctx, KZG_E_ARG, std::string(what) + row_why);
        return ready(n_cols, 32, {opts ? opts->usable : 0, opts ? opts->tail_be32 : nullptr}, LAY_READ);
    }
    uint64_t n_read() const { return blind ? blind->usable : T; }   // the rows the units read: usable, or T
    void finish(uint8_t* out_commitments48, uint64_t* out_handle) {
        if (n_out) memcpy(out_commitments48, c48, 48 * (size_t)n_out);
        *out_handle = commit();
    }
};
static const char ROW_WHY[] = ": a row must index the concatenated rows of the input sets";

// The statistics of a unit builder come back as runs of n_units u64 words; run_of[k] is the run that feeds the caller's array
// k, -1 for an array the builder fills itself
static void stats_scatter(uint64_t* const* out, const int* run_of, int n_arrays, const uint64_t* stats, uint32_t n_units) {
    for (int k = 0; k < n_arrays; k++)
        if (run_of[k] >= 0) memcpy(out[k], stats + (size_t)run_of[k] * n_units, 8 * (size_t)n_units);
}
// ec and edwards: one run means mismatches on an add or div unit and unknown op-codes on a chain; the array of the other
// meaning takes `none`
static void stats_split(uint64_t* const* out, int run, int plain, int chained, uint64_t none, const uint64_t* stats,
                        uint32_t n_units, const bool* chain) {
    for (uint32_t u = 0; u < n_units; u++) {
        const uint64_t v = stats[(size_t)run * n_units + u];
        out[plain][u] = chain[u] ? none : v;
        out[chained][u] = chain[u] ? v : none;
    }
}

int rows_open(kzg_ctx* ctx, uint32_t expect_i, uint32_t n_handles, const uint64_t* handles, uint32_t m,
              const uint8_t* points_be32, const uint32_t* masks, const uint8_t* gammas_be32, uint8_t* out_evals32,
              uint8_t* out_proofs48) {
    if (!ctx || !handles || !points_be32 || !masks || !gammas_be32 || !out_evals32 || !out_proofs48) return KZG_E_ARG;
    if (n_handles == 0 || n_handles > KZG_MAX_BATCH_OPEN)
        return fail(ctx, KZG_E_ARG, "row-set opening: the number of handles must be in [1, KZG_MAX_BATCH_OPEN]");
    if (m == 0 || m > KZG_MAX_OPEN_POINTS)
        return fail(ctx, KZG_E_ARG, "row-set opening: m must be in [1, KZG_MAX_OPEN_POINTS]");
    for (uint32_t p = 0; p < m; p++)
        if (!fr_be32_canonical(points_be32 + 32 * (size_t)p) || !fr_be32_canonical(gammas_be32 + 32 * (size_t)p))
            return fail(ctx, KZG_E_ARG, "row-set opening: points and gammas must be canonical scalars (< r)");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    RowsRefs refs{ctx};
    LaneHold H(ctx);
    if (int rc = H.take()) return rc;   // (before the lookup: an SRS load cannot free the sets' buffers under this call)
    Lane& L = H.L();
    RowTab rt;
    uint32_t k = 0, i = 0;
    uint64_t T = 0;
    if (int rc = rows_lookup(ctx, "row-set opening", expect_i, n_handles, handles, refs, rt, &k, &i, &T)) return rc;
    for (uint32_t p = 0; p < m; p++)
        if (masks[p] == 0 || (masks[p] >> k) != 0)
            return fail(ctx, KZG_E_ARG, "row-set opening: every mask must name at least one row, and rows < k only");
    int rc = check_worker(ctx, i, T);
    if (rc) return rc;
    prof_begin(ctx, L);
    rc = clear_flags(ctx, L);
    if (rc) return rc;
    return rows_open_dev(ctx, H, i, rt, k, T, m, points_be32, masks, gammas_be32, out_evals32, out_proofs48);
}

// kzg_rows_eval: the checks and lookup of kzg_rows_open without the gammas
int rows_eval(kzg_ctx* ctx, uint32_t expect_i, uint32_t n_handles, const uint64_t* handles, uint32_t m,
              const uint8_t* points_be32, const uint32_t* masks, uint8_t* out_evals32) {
    if (!ctx || !handles || !points_be32 || !masks || !out_evals32) return KZG_E_ARG;
    if (n_handles == 0 || n_handles > KZG_MAX_BATCH_OPEN)
        return fail(ctx, KZG_E_ARG, "row-set evaluation: the number of handles must be in [1, KZG_MAX_BATCH_OPEN]");
    if (m == 0 || m > KZG_MAX_OPEN_POINTS)
        return fail(ctx, KZG_E_ARG, "row-set evaluation: m must be in [1, KZG_MAX_OPEN_POINTS]");
    for (uint32_t p = 0; p < m; p++)
        if (!fr_be32_canonical(points_be32 + 32 * (size_t)p))
            return fail(ctx, KZG_E_ARG, "row-set evaluation: points must be canonical scalars (< r)");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    RowsRefs refs{ctx};
    LaneHold H(ctx);
    if (int rc = H.take()) return rc;
    Lane& L = H.L();
    RowTab rt;
    uint32_t k = 0, i = 0;
    uint64_t T = 0;
    if (int rc = rows_lookup(ctx, "row-set evaluation", expect_i, n_handles, handles, refs, rt, &k, &i, &T)) return rc;
    for (uint32_t p = 0; p < m; p++)
        if (masks[p] == 0 || (masks[p] >> k) != 0)
            return fail(ctx, KZG_E_ARG, "row-set evaluation: every mask must name at least one row, and rows < k only");
    int rc = check_worker(ctx, i, T);
    if (rc) return rc;
    prof_begin(ctx, L);
    rc = clear_flags(ctx, L);
    if (rc) return rc;
    return rows_eval_dev(ctx, H, i, rt, k, T, m, points_be32, masks, out_evals32);
}

// kzg_rows_open_lincomb: every coefficient is range-checked here, and each point's mask of nonzero coefficients built
int rows_lincomb(kzg_ctx* ctx, uint32_t expect_i, uint32_t n_handles, const uint64_t* handles, uint32_t k, uint32_t m,
                 const uint8_t* points_be32, const uint8_t* coeffs_be32, uint8_t* out_values32, uint8_t* out_proofs48) {
    if (!ctx || !handles || !points_be32 || !coeffs_be32 || !out_values32 || !out_proofs48) return KZG_E_ARG;
    if (n_handles == 0 || n_handles > KZG_MAX_BATCH_OPEN)
        return fail(ctx, KZG_E_ARG, "row-set lincomb: the number of handles must be in [1, KZG_MAX_BATCH_OPEN]");
    if (m == 0 || m > KZG_MAX_OPEN_POINTS) return fail(ctx, KZG_E_ARG, "row-set lincomb: m must be in [1, KZG_MAX_OPEN_POINTS]");
    if (k == 0 || k > KZG_MAX_BATCH_OPEN) return fail(ctx, KZG_E_ARG, "row-set lincomb: k must be in [1, KZG_MAX_BATCH_OPEN]");
    uint32_t masks[KZG_MAX_OPEN_POINTS] = {};
    static const uint8_t zero[32] = {};
    for (uint32_t p = 0; p < m; p++) {
        if (!fr_be32_canonical(points_be32 + 32 * (size_t)p))
            return fail(ctx, KZG_E_ARG, "row-set lincomb: points must be canonical scalars (< r)");
        for (uint32_t j = 0; j < k; j++) {
            const uint8_t* c = coeffs_be32 + 32 * ((size_t)p * k + j);
            if (!fr_be32_canonical(c)) return fail(ctx, KZG_E_ARG, "row-set lincomb: coefficients must be canonical scalars (< r)");
            if (memcmp(c, zero, 32) != 0) masks[p] |= 1u << j;
        }
        if (!masks[p]) return fail(ctx, KZG_E_ARG, "row-set lincomb: every point needs a nonzero coefficient");
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    RowsRefs refs{ctx};
    LaneHold H(ctx);
    if (int rc = H.take()) return rc;
    Lane& L = H.L();
    RowTab rt;
    uint32_t nrows = 0, i = 0;
    uint64_t T = 0;
    if (int rc = rows_lookup(ctx, "row-set lincomb", expect_i, n_handles, handles, refs, rt, &nrows, &i, &T)) return rc;
    if (nrows != k) return fail(ctx, KZG_E_ARG, "row-set lincomb: k must equal the rows of the concatenated sets");
    int rc = check_worker(ctx, i, T);
    if (rc) return rc;
    prof_begin(ctx, L);
    rc = clear_flags(ctx, L);
    if (rc) return rc;
    return rows_lincomb_dev(ctx, H, i, rt, k, T, m, points_be32, coeffs_be32, masks, out_values32, out_proofs48);
}

// kzg_rows_commit_shplonk: the argument checks, the rows' point sets grouped (rows with c_j = 0 left out), the lookups of an
// open and the reservation of a commit
static_assert(KZG_MAX_SHPLONK_ROWS + 1 <= KZG_MAX_BATCH_OPEN && KZG_MAX_SHPLONK_POINTS <= 8, "round B opens k + 1 rows; a "
              "point set is a byte");
int rows_shplonk(kzg_ctx* ctx, uint32_t expect_i, uint32_t n_handles, const uint64_t* handles, uint32_t k, uint32_t m,
                 const uint8_t* points_be32, const uint32_t* masks, const uint8_t* coeffs_be32, uint8_t* out_commitment48,
                 uint64_t* out_handle) {
    if (!ctx || !handles || !points_be32 || !masks || !coeffs_be32 || !out_commitment48 || !out_handle) return KZG_E_ARG;
    if (n_handles == 0 || n_handles > KZG_MAX_BATCH_OPEN)
        return fail(ctx, KZG_E_ARG, "shplonk: the number of handles must be in [1, KZG_MAX_BATCH_OPEN]");
    if (k == 0 || k > KZG_MAX_SHPLONK_ROWS) return fail(ctx, KZG_E_ARG, "shplonk: k must be in [1, KZG_MAX_SHPLONK_ROWS]");
    if (m == 0 || m > KZG_MAX_SHPLONK_POINTS) return fail(ctx, KZG_E_ARG, "shplonk: m must be in [1, KZG_MAX_SHPLONK_POINTS]");
    static const uint8_t zero[32] = {};
    for (uint32_t p = 0; p < m; p++) {
        if (!fr_be32_canonical(points_be32 + 32 * (size_t)p))
            return fail(ctx, KZG_E_ARG, "shplonk: points must be canonical scalars (< r)");
        for (uint32_t q = 0; q < p; q++)
            if (memcmp(points_be32 + 32 * (size_t)p, points_be32 + 32 * (size_t)q, 32) == 0)
                return fail(ctx, KZG_E_ARG, "shplonk: the points must be pairwise distinct");
        if ((masks[p] >> k) != 0) return fail(ctx, KZG_E_ARG, "shplonk: a mask names a row >= k");
    }
    ShGroup groups[KZG_MAX_SHPLONK_ROWS];
    uint32_t n_groups = 0, max_pts = 0;
    for (uint32_t j = 0; j < k; j++) {
        const uint8_t* c = coeffs_be32 + 32 * (size_t)j;
        if (!fr_be32_canonical(c)) return fail(ctx, KZG_E_ARG, "shplonk: coefficients must be canonical scalars (< r)");
        if (memcmp(c, zero, 32) == 0) continue;   // the row is left out, whatever its mask
        ShGroup g = {};
        for (uint32_t p = 0; p < m; p++)
            if ((masks[p] >> j) & 1u) g.pt[g.npts++] = (uint8_t)p;
        if (!g.npts) return fail(ctx, KZG_E_ARG, "shplonk: a row with a nonzero coefficient is opened at no point");
        uint32_t t = 0;
        while (t < n_groups && !(groups[t].npts == g.npts && memcmp(groups[t].pt, g.pt, g.npts) == 0)) t++;
        if (t == n_groups) groups[n_groups++] = g;
        groups[t].rows |= 1u << j;
        max_pts = std::max<uint32_t>(max_pts, g.npts);
    }
    if (!n_groups) return fail(ctx, KZG_E_ARG, "shplonk: every coefficient is zero");
    std::stable_sort(groups, groups + n_groups, [](const ShGroup& a, const ShGroup& b) { return a.npts > b.npts; });
    HIPCHK(ctx, hipSetDevice(ctx->device));
    RowsPending pend{ctx};
    RowsRefs refs{ctx};
    LaneHold H(ctx);
    if (int rc = H.take()) return rc;   // (before the lookup: an SRS load cannot free the sets' buffers under this call)
    Lane& L = H.L();
    RowTab rt;
    uint32_t nrows = 0, i = 0;
    uint64_t T = 0;
    if (int rc = rows_lookup(ctx, "shplonk", expect_i, n_handles, handles, refs, rt, &nrows, &i, &T)) return rc;
    if (nrows != k) return fail(ctx, KZG_E_ARG, "shplonk: k must equal the rows of the concatenated sets");
    int rc = check_worker(ctx, i, T);
    if (rc) return rc;
    if (max_pts >= T) return fail(ctx, KZG_E_ARG, "shplonk: a row is opened at T or more points (its quotient is zero)");
    if (int rc2 = rows_reserve(ctx, "shplonk", pend, (size_t)T * 32)) return rc2;
    prof_begin(ctx, L);
    rc = clear_flags(ctx, L);
    if (rc) return rc;
    uint8_t c48[48];
    rc = rows_shplonk_dev(ctx, H, i, rt, k, T, m, points_be32, coeffs_be32, n_groups, groups, pend.buf.as<uint32_t>(), c48);
    if (rc) return rc;
    memcpy(out_commitment48, c48, 48);
    *out_handle = rows_insert(ctx, pend, i, 1, T);
    return KZG_OK;
}

// the blinding rows of a _zk builder against the row length, once that is known: 1 <= usable <= T - 1, at most
// KZG_MAX_BLIND_ROWS rows from `usable` on, T - usable - 1 canonical tail scalars (none: the pointer may be null)
static_assert(KZG_MAX_BLIND_ROWS == BLIND_MAX_ROWS, "the header's cap is the kernels' cap");
static int blind_check(kzg_ctx* ctx, const char* what, uint64_t T, const Blind& zk) {
    auto bad = [&](const char* why) { return fail(ctx, KZG_E_ARG, std::string(what) + why); };
    if (zk.usable == 0 || zk.usable >= T) return bad(": usable must be in [1, T - 1]");
    if (T - zk.usable > KZG_MAX_BLIND_ROWS) return bad(": at most KZG_MAX_BLIND_ROWS rows may lie at or behind row `usable`");
    const uint64_t n_tail = T - zk.usable - 1;
    if (n_tail && !zk.tail_be32) return bad(": tail_be32 may be null only when usable = T - 1");
    for (uint64_t j = 0; j < n_tail; j++)
        if (!fr_be32_canonical(zk.tail_be32 + 32 * (size_t)j)) return bad(": tail scalars must be canonical (< r)");
    return KZG_OK;
}

// kzg_rows_commit_grand_product: the lookups of an open (two handle lists), the reservation of a commit.  zk: the blinding
// rows of kzg_rows_commit_grand_product_zk (null: the plain call).  start_be32: kzg_rows_commit_grand_product_chain's start of
// z instead of 1 (null: not a chain)
int rows_grand_product(kzg_ctx* ctx, uint32_t expect_i, uint32_t n_wire_handles, const uint64_t* wire_handles,
                       uint32_t n_sigma_handles, const uint64_t* sigma_handles, uint32_t k, const uint8_t* shifts_be32,
                       const uint8_t* beta_be32, const uint8_t* gamma_be32, uint8_t* out_commitment48, uint8_t* out_closing32,
                       uint64_t* out_handle, const Blind* zk, const uint8_t* start_be32) {
    if (!ctx || !wire_handles || !sigma_handles || !shifts_be32 || !beta_be32 || !gamma_be32 || !out_commitment48 ||
        !out_closing32 || !out_handle)
        return KZG_E_ARG;
    static const uint8_t zero32[32] = {};
    if (start_be32 && (!fr_be32_canonical(start_be32) || memcmp(start_be32, zero32, 32) == 0))
        return fail(ctx, KZG_E_ARG, "grand product: start must be a canonical scalar (< r) other than 0");
    if (n_wire_handles == 0 || n_wire_handles > KZG_MAX_BATCH_OPEN || n_sigma_handles == 0 || n_sigma_handles > KZG_MAX_BATCH_OPEN)
        return fail(ctx, KZG_E_ARG, "grand product: the number of handles in each list must be in [1, KZG_MAX_BATCH_OPEN]");
    if (k == 0 || k > KZG_MAX_BATCH_OPEN) return fail(ctx, KZG_E_ARG, "grand product: k must be in [1, KZG_MAX_BATCH_OPEN]");
    if (!fr_be32_canonical(beta_be32) || !fr_be32_canonical(gamma_be32))
        return fail(ctx, KZG_E_ARG, "grand product: beta and gamma must be canonical scalars (< r)");
    for (uint32_t j = 0; j < k; j++)
        if (!fr_be32_canonical(shifts_be32 + 32 * (size_t)j))
            return fail(ctx, KZG_E_ARG, "grand product: shifts must be canonical scalars (< r)");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    RowsPending pend{ctx};
    RowsRefs wrefs{ctx}, srefs{ctx};
    LaneHold H(ctx);
    if (int rc = H.take()) return rc;   // (before the lookups: an SRS load cannot free the sets' buffers under this call)
    Lane& L = H.L();
    RowTab wt, st;
    uint32_t kw = 0, ks = 0, i = 0, is = 0;
    uint64_t T = 0, Ts = 0;
    if (int rc = rows_lookup(ctx, "grand product (wires)", expect_i, n_wire_handles, wire_handles, wrefs, wt, &kw, &i, &T)) return rc;
    if (int rc = rows_lookup(ctx, "grand product (sigmas)", expect_i, n_sigma_handles, sigma_handles, srefs, st, &ks, &is, &Ts))
        return rc;
    if (is != i || Ts != T) return fail(ctx, KZG_E_ARG, "grand product: all sets must belong to one worker and have one row length");
    if (kw != k || ks != k)
        return fail(ctx, KZG_E_ARG, "grand product: the wire sets and the sigma sets must each hold exactly k rows");
    int rc = check_worker(ctx, i, T);
    if (rc) return rc;
    if (ilog2_exact(T) < 0) return fail(ctx, KZG_E_ARG, "grand product: the row length must be a power of two");
    if (zk)
        if (int rcz = blind_check(ctx, "grand product", T, *zk)) return rcz;
    if (int rc2 = rows_reserve(ctx, "grand product", pend, (size_t)T * 32)) return rc2;
    prof_begin(ctx, L);
    rc = clear_flags(ctx, L);
    if (rc) return rc;
    bool zero_den = false;
    uint8_t c48[48], closing[32];
    rc = rows_grand_product_dev(ctx, H, i, wt, st, k, T, shifts_be32, beta_be32, gamma_be32, pend.buf.as<uint32_t>(), c48, closing,
                                &zero_den, zk, start_be32);
    if (rc) return rc;
    if (zero_den)
        return fail(ctx, KZG_E_ARG, zk ? "grand product: zero denominator (some a_j + beta sigma_j + gamma vanishes on a usable "
                                         "row): z is undefined, no set was created"
                                       : "grand product: zero denominator (some a_j + beta sigma_j + gamma vanishes on the domain): "
                                         "z is undefined, no set was created");
    memcpy(out_commitment48, c48, 48);
    memcpy(out_closing32, closing, 32);
    *out_handle = rows_insert(ctx, pend, i, 1, T);
    return KZG_OK;
}

// kzg_rows_commit_shuffle: the lookups of an open (two handle lists, and the selectors' when opts names some), the
// reservation of a commit.  opts == NULL, or usable == 0 and no selector index list: the plain call
int rows_shuffle(kzg_ctx* ctx, uint32_t expect_i, uint32_t n_input_handles, const uint64_t* input_handles,
                 uint32_t n_shuffle_handles, const uint64_t* shuffle_handles, uint32_t n_groups, uint32_t width,
                 const uint8_t* theta_be32, const uint8_t* gamma_be32, const kzg_shuffle_opts* opts, uint8_t* out_commitment48,
                 uint8_t* out_closing32, uint64_t* out_handle) {
    if (!ctx || !input_handles || !shuffle_handles || !theta_be32 || !gamma_be32 || !out_commitment48 || !out_closing32 ||
        !out_handle)
        return KZG_E_ARG;
    const bool has_sel = opts && (opts->input_sel || opts->shuffle_sel);
    if (opts && opts->n_sel_handles && !opts->sel_handles) return KZG_E_ARG;
    if (opts && opts->n_sel_handles > KZG_MAX_BATCH_OPEN)
        return fail(ctx, KZG_E_ARG, "shuffle: at most KZG_MAX_BATCH_OPEN selector handles");
    if (n_input_handles == 0 || n_input_handles > KZG_MAX_BATCH_OPEN || n_shuffle_handles == 0 ||
        n_shuffle_handles > KZG_MAX_BATCH_OPEN)
        return fail(ctx, KZG_E_ARG, "shuffle: the number of handles in each list must be in [1, KZG_MAX_BATCH_OPEN]");
    if (n_groups == 0 || width == 0 || (uint64_t)n_groups * width > KZG_MAX_BATCH_OPEN)
        return fail(ctx, KZG_E_ARG, "shuffle: n_groups and width must be at least 1 and n_groups * width at most "
                                    "KZG_MAX_BATCH_OPEN");
    if (!fr_be32_canonical(theta_be32) || !fr_be32_canonical(gamma_be32))
        return fail(ctx, KZG_E_ARG, "shuffle: theta and gamma must be canonical scalars (< r)");
    if (has_sel && !opts->n_sel_handles)
        for (uint32_t g = 0; g < n_groups; g++)
            if ((opts->input_sel && opts->input_sel[g] != KZG_NO_SELECTOR) ||
                (opts->shuffle_sel && opts->shuffle_sel[g] != KZG_NO_SELECTOR))
                return fail(ctx, KZG_E_ARG, "shuffle: a selector index was given but no selector handles");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    RowsPending pend{ctx};
    RowsRefs irefs{ctx}, srefs{ctx}, qrefs{ctx};
    LaneHold H(ctx);
    if (int rc = H.take()) return rc;   // (before the lookups: an SRS load cannot free the sets' buffers under this call)
    Lane& L = H.L();
    RowTab it, st, qt;
    uint32_t ki = 0, ks = 0, kq = 0, i = 0, i2 = 0;
    uint64_t T = 0, T2 = 0;
    if (int rc = rows_lookup(ctx, "shuffle (inputs)", expect_i, n_input_handles, input_handles, irefs, it, &ki, &i, &T)) return rc;
    if (int rc = rows_lookup(ctx, "shuffle (shuffles)", expect_i, n_shuffle_handles, shuffle_handles, srefs, st, &ks, &i2, &T2))
        return rc;
    if (i2 != i || T2 != T) return fail(ctx, KZG_E_ARG, "shuffle: all sets must belong to one worker and have one row length");
    if (opts && opts->n_sel_handles) {
        if (int rc = rows_lookup(ctx, "shuffle (selectors)", expect_i, opts->n_sel_handles, opts->sel_handles, qrefs, qt, &kq, &i2, &T2))
            return rc;
        if (i2 != i || T2 != T) return fail(ctx, KZG_E_ARG, "shuffle: all sets must belong to one worker and have one row length");
    }
    if (ki != n_groups * width || ks != n_groups * width)
        return fail(ctx, KZG_E_ARG, "shuffle: the input sets and the shuffle sets must each hold exactly n_groups * width rows");
    ShuffleSel sel;
    memset(&sel, 0, sizeof(sel));
    bool any_sel = false;   // (every entry KZG_NO_SELECTOR: the call without selectors)
    for (uint32_t g = 0; has_sel && g < n_groups; g++) {
        const uint32_t ji = opts->input_sel ? opts->input_sel[g] : KZG_NO_SELECTOR;
        const uint32_t js = opts->shuffle_sel ? opts->shuffle_sel[g] : KZG_NO_SELECTOR;
        if ((ji != KZG_NO_SELECTOR && ji >= kq) || (js != KZG_NO_SELECTOR && js >= kq))
            return fail(ctx, KZG_E_ARG, "shuffle: an input_sel / shuffle_sel entry must be KZG_NO_SELECTOR or index the "
                                        "concatenated rows of the selector sets");
        if (ji != KZG_NO_SELECTOR) sel.in[g] = qt.r[ji];
        if (js != KZG_NO_SELECTOR) sel.sh[g] = qt.r[js];
        any_sel = any_sel || sel.in[g] || sel.sh[g];
    }
    int rc = check_worker(ctx, i, T);
    if (rc) return rc;
    if (ilog2_exact(T) < 0) return fail(ctx, KZG_E_ARG, "shuffle: the row length must be a power of two");
    const Blind zk = {opts ? opts->usable : 0, opts ? opts->tail_be32 : nullptr};
    if (zk.usable) {
        if (int rcz = blind_check(ctx, "shuffle", T, zk)) return rcz;
    } else if (zk.tail_be32) {
        return fail(ctx, KZG_E_ARG, "shuffle: tail_be32 must be null in the plain layout (usable = 0)");
    }
    if (int rc2 = rows_reserve(ctx, "shuffle", pend, (size_t)T * 32)) return rc2;
    prof_begin(ctx, L);
    rc = clear_flags(ctx, L);
    if (rc) return rc;
    bool zero_den = false;
    uint8_t c48[48], closing[32];
    rc = rows_shuffle_dev(ctx, H, i, it, st, n_groups, width, T, theta_be32, gamma_be32, pend.buf.as<uint32_t>(), c48, closing,
                          &zero_den, zk.usable ? &zk : nullptr, any_sel ? &sel : nullptr);
    if (rc) return rc;
    if (zero_den)
        return fail(ctx, KZG_E_ARG, zk.usable ? "shuffle: zero denominator (some shuffle-side factor vanishes on a usable row): z is "
                                                "undefined, no set was created"
                                              : "shuffle: zero denominator (some shuffle-side factor vanishes on the domain): z is "
                                                "undefined, no set was created");
    memcpy(out_commitment48, c48, 48);
    memcpy(out_closing32, closing, 32);
    *out_handle = rows_insert(ctx, pend, i, 1, T);
    return KZG_OK;
}

// kzg_rows_commit_sorted: the lookups of an open (one handle list), the reservation of a commit of `width` rows.  opts == NULL,
// or usable == 0: all T rows are sorted
int rows_sorted(kzg_ctx* ctx, uint32_t expect_i, uint32_t n_input_handles, const uint64_t* input_handles, uint32_t width,
                uint32_t n_keys, const kzg_sorted_opts* opts, uint8_t* out_commitments48, uint64_t* out_handle) {
    if (!ctx || !input_handles || !out_commitments48 || !out_handle) return KZG_E_ARG;
    if (n_input_handles == 0 || n_input_handles > KZG_MAX_BATCH_OPEN)
        return fail(ctx, KZG_E_ARG, "sorted: the number of handles must be in [1, KZG_MAX_BATCH_OPEN]");
    if (width == 0 || width > KZG_MAX_BATCH_OPEN) return fail(ctx, KZG_E_ARG, "sorted: width must be in [1, KZG_MAX_BATCH_OPEN]");
    if (n_keys == 0 || n_keys > width) return fail(ctx, KZG_E_ARG, "sorted: n_keys must be in [1, width]");
    BuilderCall C(ctx, "sorted");
    RowTab it;
    uint32_t ki = 0;
    if (int rc = C.begin("sorted", expect_i, n_input_handles, input_handles, it, &ki)) return rc;
    if (ki != width) return fail(ctx, KZG_E_ARG, "sorted: the input sets must hold exactly width rows");
    // (2^27: row indices and slot offsets are u32, 256 counts per tile of the passes)
    if (int rc = C.ready(width, 27, {opts ? opts->usable : 0, opts ? opts->tail_be32 : nullptr}, LAY_SORTED)) return rc;
    uint8_t c48[KZG_MAX_BATCH_OPEN * 48];
    if (int rc = rows_sorted_dev(ctx, C.H, C.i, it, width, n_keys, C.T, C.dst(), c48, C.blind)) return rc;
    memcpy(out_commitments48, c48, 48 * (size_t)width);
    *out_handle = C.commit();
    return KZG_OK;
}

// what kzg_rows_commit_sigma and kzg_rows_check_copies ask of their opts once T is known: *n <- the rows that take part
static int sigma_layout(kzg_ctx* ctx, const char* what, const kzg_sigma_opts* opts, uint32_t k, uint64_t T, uint64_t* n) {
    const char* why = nullptr;
    *n = opts && opts->usable ? opts->usable : T;
    if (ilog2_exact(T) < 0) why = "the row length must be a power of two";
    else if (*n >= T && opts && opts->usable) why = "usable must be in [1, T - 1] (0: all T rows take part)";
    else if (opts && opts->free_label_be32 && !fr_be32_canonical(opts->free_label_be32))
        why = "the free label must be a canonical scalar (< r)";
    else if (*n > ((uint64_t)1 << 27) || (uint64_t)k * *n > ((uint64_t)1 << 27))   // positions of the sort are u32
        why = "k * n cells take part, which must be at most 2^27";
    return why ? fail(ctx, KZG_E_ARG, std::string(what) + ": " + why) : KZG_OK;
}

// kzg_rows_commit_sigma: the lookups of an open (one handle list), the reservation of a commit of k rows.  opts == NULL: plain
// layout, no free label.  The shifts and the free label are checked here, on the host (the kernels check them again)
int rows_sigma(kzg_ctx* ctx, uint32_t expect_i, uint32_t n_label_handles, const uint64_t* label_handles, uint32_t k,
               const uint8_t* shifts_be32, const kzg_sigma_opts* opts, uint8_t* out_commitments48, uint64_t* out_stats,
               uint64_t* out_handle) {
    if (!ctx || !label_handles || !shifts_be32 || !out_commitments48 || !out_stats || !out_handle) return KZG_E_ARG;
    if (n_label_handles == 0 || n_label_handles > KZG_MAX_BATCH_OPEN)
        return fail(ctx, KZG_E_ARG, "sigma: the number of handles must be in [1, KZG_MAX_BATCH_OPEN]");
    if (k == 0 || k > KZG_MAX_BATCH_OPEN) return fail(ctx, KZG_E_ARG, "sigma: k must be in [1, KZG_MAX_BATCH_OPEN]");
    for (uint32_t c = 0; c < k; c++)
        if (!fr_be32_canonical(shifts_be32 + 32 * (size_t)c))
            return fail(ctx, KZG_E_ARG, "sigma: the shifts must be canonical scalars (< r)");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    RowsPending pend{ctx};
    RowsRefs lrefs{ctx};
    LaneHold H(ctx);
    if (int rc = H.take()) return rc;   // (before the lookups: an SRS load cannot free the sets' buffers under this call)
    Lane& L = H.L();
    RowTab lt;
    uint32_t kl = 0, i = 0;
    uint64_t T = 0, n = 0;
    if (int rc = rows_lookup(ctx, "sigma", expect_i, n_label_handles, label_handles, lrefs, lt, &kl, &i, &T)) return rc;
    if (kl != k) return fail(ctx, KZG_E_ARG, "sigma: the label sets must hold exactly k rows");
    int rc = check_worker(ctx, i, T);
    if (rc) return rc;
    if (int rc2 = sigma_layout(ctx, "sigma", opts, k, T, &n)) return rc2;
    if (int rc2 = rows_reserve(ctx, "sigma", pend, (size_t)k * T * 32)) return rc2;
    prof_begin(ctx, L);
    rc = clear_flags(ctx, L);
    if (rc) return rc;
    uint8_t c48[KZG_MAX_BATCH_OPEN * 48];
    uint64_t stats[2];
    rc = rows_sigma_dev(ctx, H, i, lt, k, T, n, shifts_be32, opts ? opts->free_label_be32 : nullptr, pend.buf.as<uint32_t>(), c48,
                        stats);
    if (rc) return rc;
    memcpy(out_commitments48, c48, 48 * (size_t)k);
    out_stats[0] = stats[0];
    out_stats[1] = stats[1];
    *out_handle = rows_insert(ctx, pend, i, k, T);
    return KZG_OK;
}

// kzg_rows_check_copies: the lookups of an open (two handle lists, as rows_fetch); no reservation, no set
int rows_check_copies(kzg_ctx* ctx, uint32_t expect_i, uint32_t n_wire_handles, const uint64_t* wire_handles,
                      uint32_t n_label_handles, const uint64_t* label_handles, uint32_t k, const kzg_sigma_opts* opts,
                      uint64_t* out) {
    if (!ctx || !wire_handles || !label_handles || !out) return KZG_E_ARG;
    if (n_wire_handles == 0 || n_wire_handles > KZG_MAX_BATCH_OPEN || n_label_handles == 0 || n_label_handles > KZG_MAX_BATCH_OPEN)
        return fail(ctx, KZG_E_ARG, "check_copies: the number of handles in each list must be in [1, KZG_MAX_BATCH_OPEN]");
    if (k == 0 || k > KZG_MAX_BATCH_OPEN) return fail(ctx, KZG_E_ARG, "check_copies: k must be in [1, KZG_MAX_BATCH_OPEN]");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    RowsRefs wrefs{ctx}, lrefs{ctx};
    LaneHold H(ctx);
    if (int rc = H.take()) return rc;   // (before the lookups: an SRS load cannot free the sets' buffers under this call)
    Lane& L = H.L();
    RowTab wt, lt;
    uint32_t kw = 0, kl = 0, i = 0, i2 = 0;
    uint64_t T = 0, T2 = 0, n = 0;
    if (int rc = rows_lookup(ctx, "check_copies: wires", expect_i, n_wire_handles, wire_handles, wrefs, wt, &kw, &i, &T)) return rc;
    if (int rc = rows_lookup(ctx, "check_copies: labels", expect_i, n_label_handles, label_handles, lrefs, lt, &kl, &i2, &T2))
        return rc;
    if (i2 != i || T2 != T) return fail(ctx, KZG_E_ARG, "check_copies: all sets must belong to one worker and have one row length");
    if (kw != k || kl != k) return fail(ctx, KZG_E_ARG, "check_copies: the wire sets and the label sets must hold exactly k rows each");
    int rc = check_worker(ctx, i, T);
    if (rc) return rc;
    if (int rc2 = sigma_layout(ctx, "check_copies", opts, k, T, &n)) return rc2;
    prof_begin(ctx, L);
    rc = clear_flags(ctx, L);
    if (rc) return rc;
    uint64_t res[2];
    rc = rows_check_copies_dev(ctx, H, i, wt, lt, k, T, n, opts ? opts->free_label_be32 : nullptr, res);
    if (rc) return rc;
    out[0] = res[0];
    out[1] = res[1];
    return KZG_OK;
}

// kzg_rows_commit_derived: the lookups of an open (one handle list), the reservation of a commit of n_out rows.  opts == NULL,
// or usable == 0: all T rows are read
int rows_derived(kzg_ctx* ctx, uint32_t expect_i, uint32_t n_input_handles, const uint64_t* input_handles, uint32_t n_ops,
                 const kzg_derive_op* ops, const kzg_derive_opts* opts, uint8_t* out_commitments48, uint64_t* out_counts,
                 uint64_t* out_handle) {
    if (!ctx || !input_handles || !out_commitments48 || !out_counts || !out_handle) return KZG_E_ARG;
    if (n_input_handles == 0 || n_input_handles > KZG_MAX_BATCH_OPEN)
        return fail(ctx, KZG_E_ARG, "derived: the number of handles must be in [1, KZG_MAX_BATCH_OPEN]");
    if (n_ops == 0 || !ops) return fail(ctx, KZG_E_ARG, "derived: n_ops must be at least 1");
    uint64_t n_out = 0;
    for (uint32_t o = 0; o < n_ops && n_out <= KZG_MAX_BATCH_OPEN; o++) {
        const kzg_derive_op& op = ops[o];
        if (op.kind == KZG_DERIVE_INV0) {
            if (op.bits != 0) return fail(ctx, KZG_E_ARG, "derived: bits must be 0 on an INV0 op");
            if (op.count != 1 && op.count != 2)
                return fail(ctx, KZG_E_ARG, "derived: count must be 1 or 2 on an INV0 op (inv0, then the is-zero bit)");
        } else if (op.kind == KZG_DERIVE_LIMBS) {
            if (op.bits == 0 || op.bits > 32) return fail(ctx, KZG_E_ARG, "derived: bits must be in [1, 32] on a LIMBS op");
            if (op.count == 0 || op.count > KZG_MAX_BATCH_OPEN)
                return fail(ctx, KZG_E_ARG, "derived: count must be in [1, KZG_MAX_BATCH_OPEN] on a LIMBS op");
            if ((uint64_t)op.bits * op.count > 256) return fail(ctx, KZG_E_ARG, "derived: bits * count must be at most 256");
        } else {
            return fail(ctx, KZG_E_ARG, "derived: unknown kind (KZG_DERIVE_INV0 or KZG_DERIVE_LIMBS)");
        }
        n_out += op.count;
    }
    if (n_out > KZG_MAX_BATCH_OPEN)
        return fail(ctx, KZG_E_ARG, "derived: n_out, the sum of the counts, must be in [1, KZG_MAX_BATCH_OPEN]");
    BuilderCall C(ctx, "derived");
    RowTab it;
    uint32_t ki = 0;
    if (int rc = C.begin("derived", expect_i, n_input_handles, input_handles, it, &ki)) return rc;
    for (uint32_t o = 0; o < n_ops; o++)
        if (ops[o].row >= ki) return fail(ctx, KZG_E_ARG, "derived: a row must index the concatenated rows of the input sets");
    if (int rc = C.ready((uint32_t)n_out, 0, {opts ? opts->usable : 0, opts ? opts->tail_be32 : nullptr}, LAY_READ)) return rc;
    uint8_t c48[KZG_MAX_BATCH_OPEN * 48];
    uint64_t counts[KZG_MAX_BATCH_OPEN];
    if (int rc = rows_derived_dev(ctx, C.H, C.i, it, n_ops, ops, C.n_out, C.T, C.dst(), c48, counts, C.blind)) return rc;
    memcpy(out_commitments48, c48, 48 * (size_t)n_out);
    memcpy(out_counts, counts, 8 * (size_t)n_ops);
    *out_handle = C.commit();
    return KZG_OK;
}

// kzg_rows_commit_int: the lookups of an open (one handle list), the reservation of a commit of n_out rows.  opts == NULL, or
// usable == 0: all T rows are read.  Kinds, widths, counts and immediates are checked here, on the host, before a lane is taken
int rows_int(kzg_ctx* ctx, uint32_t expect_i, uint32_t n_input_handles, const uint64_t* input_handles, uint32_t n_ops,
             const kzg_int_op* ops, const kzg_derive_opts* opts, uint8_t* out_commitments48, uint64_t* out_counts,
             uint64_t* out_first, uint64_t* out_handle) {
    if (!ctx || !input_handles || !out_commitments48 || !out_counts || !out_first || !out_handle) return KZG_E_ARG;
    if (n_input_handles == 0 || n_input_handles > KZG_MAX_BATCH_OPEN)
        return fail(ctx, KZG_E_ARG, "int: the number of handles must be in [1, KZG_MAX_BATCH_OPEN]");
    if (n_ops == 0 || n_ops > KZG_MAX_BATCH_OPEN || !ops)
        return fail(ctx, KZG_E_ARG, "int: n_ops must be in [1, KZG_MAX_BATCH_OPEN]");
    uint32_t n_out = 0;
    for (uint32_t o = 0; o < n_ops; o++) {
        const kzg_int_op& op = ops[o];
        if (op.kind < KZG_INT_AND || op.kind > KZG_INT_SPLIT)
            return fail(ctx, KZG_E_ARG, "int: unknown kind (KZG_INT_AND .. KZG_INT_SPLIT)");
        if (op.flags & ~KZG_INT_IMM) return fail(ctx, KZG_E_ARG, "int: flags must be 0 or KZG_INT_IMM");
        if (op.width == 0 || op.width > 64) return fail(ctx, KZG_E_ARG, "int: the width must be in [1, 64]");
        if (op.count != 1 && !(op.count == 2 && op.kind >= KZG_INT_ADD))
            return fail(ctx, KZG_E_ARG, "int: count must be 1 on AND, OR and XOR, and 1 or 2 on the other kinds");
        if (op.flags & KZG_INT_IMM) {
            if (op.b != 0) return fail(ctx, KZG_E_ARG, "int: the row b must be 0 beside an immediate");
            if (op.kind == KZG_INT_SPLIT ? op.imm > op.width : op.width < 64 && (op.imm >> op.width) != 0)
                return fail(ctx, KZG_E_ARG, "int: an immediate must be below 2^width (SPLIT: a shift of at most width)");
        } else if (op.imm != 0) {
            return fail(ctx, KZG_E_ARG, "int: the immediate must be 0 without KZG_INT_IMM");
        }
        n_out += op.count;
    }
    if (n_out > KZG_MAX_BATCH_OPEN)
        return fail(ctx, KZG_E_ARG, "int: n_out, the sum of the counts, must be in [1, KZG_MAX_BATCH_OPEN]");
    BuilderCall C(ctx, "int");
    RowTab it;
    uint32_t ki = 0;
    if (int rc = C.begin("int", expect_i, n_input_handles, input_handles, it, &ki)) return rc;
    for (uint32_t o = 0; o < n_ops; o++)
        if (ops[o].a >= ki || ops[o].b >= ki)
            return fail(ctx, KZG_E_ARG, "int: a row must index the concatenated rows of the input sets");
    if (int rc = C.ready(n_out, 0, {opts ? opts->usable : 0, opts ? opts->tail_be32 : nullptr}, LAY_READ)) return rc;
    uint8_t c48[KZG_MAX_BATCH_OPEN * 48];
    uint64_t counts[KZG_MAX_BATCH_OPEN], first[KZG_MAX_BATCH_OPEN];
    if (int rc = rows_int_dev(ctx, C.H, C.i, it, n_ops, ops, n_out, C.T, C.dst(), c48, counts, first, C.blind)) return rc;
    memcpy(out_commitments48, c48, 48 * (size_t)n_out);
    memcpy(out_counts, counts, 8 * (size_t)n_ops);
    memcpy(out_first, first, 8 * (size_t)n_ops);
    *out_handle = C.commit();
    return KZG_OK;
}

// kzg_rows_commit_alu: a BuilderCall around its own checks.  The program and the units are checked here, on the host, before a lane is taken
int rows_alu(kzg_ctx* ctx, uint32_t expect_i, uint32_t n_input_handles, const uint64_t* input_handles, uint32_t n_entries,
             const kzg_alu_entry* program, uint32_t n_units, const kzg_alu_unit* units, const kzg_derive_opts* opts,
             uint8_t* out_commitments48, uint64_t* out_counts, uint64_t* out_first, uint64_t* out_unknown,
             uint64_t* out_first_unknown, uint64_t* out_handle) {
    if (!ctx || !input_handles || !out_commitments48 || !out_counts || !out_first || !out_unknown || !out_first_unknown ||
        !out_handle)
        return KZG_E_ARG;
    if (n_input_handles == 0 || n_input_handles > KZG_MAX_BATCH_OPEN)
        return fail(ctx, KZG_E_ARG, "alu: the number of handles must be in [1, KZG_MAX_BATCH_OPEN]");
    if (n_entries == 0 || n_entries > KZG_ALU_MAX_PROGRAM || !program)
        return fail(ctx, KZG_E_ARG, "alu: n_entries must be in [1, KZG_ALU_MAX_PROGRAM]");
    if (n_units == 0 || n_units > KZG_ALU_MAX_UNITS || !units)
        return fail(ctx, KZG_E_ARG, "alu: n_units must be in [1, KZG_ALU_MAX_UNITS]");
    bool two_rows = false;
    for (uint32_t e = 0; e < n_entries; e++) {
        const kzg_alu_entry& en = program[e];
        if (en.kind > KZG_ALU_SEXT) return fail(ctx, KZG_E_ARG, "alu: unknown kind (KZG_ALU_IDLE, KZG_ALU_AND .. KZG_ALU_SEXT)");
        if (en.pad != 0) return fail(ctx, KZG_E_ARG, "alu: an entry's pad must be 0");
        if (en.kind == KZG_ALU_IDLE) {
            if (en.width != 0 || en.imm != 0 || en.flags != 0)
                return fail(ctx, KZG_E_ARG, "alu: an idle entry must have width, imm and flags 0");
            continue;
        }
        if (en.flags & ~KZG_ALU_IMM) return fail(ctx, KZG_E_ARG, "alu: flags must be 0 or KZG_ALU_IMM");
        if (en.width == 0 || en.width > 64) return fail(ctx, KZG_E_ARG, "alu: the width must be in [1, 64]");
        if (en.flags & KZG_ALU_IMM) {
            const bool field = en.kind == KZG_ALU_SPLIT || en.kind == KZG_ALU_SEXT;
            if (field ? en.imm > en.width || (en.kind == KZG_ALU_SEXT && en.imm == 0) : en.width < 64 && (en.imm >> en.width) != 0)
                return fail(ctx, KZG_E_ARG,
                            "alu: an immediate must be below 2^width (SPLIT, SEXT: at most width; SEXT: at least 1)");
        } else if (en.imm != 0) {
            return fail(ctx, KZG_E_ARG, "alu: the immediate must be 0 without KZG_ALU_IMM");
        }
        two_rows |= en.kind > KZG_ALU_XOR;
    }
    uint32_t n_out = 0;
    for (uint32_t u = 0; u < n_units; u++) {
        if (units[u].count != 1 && !(units[u].count == 2 && two_rows))
            return fail(ctx, KZG_E_ARG, "alu: count must be 1 or 2, and 1 where no entry's kind has a second row (AND, OR, XOR)");
        n_out += units[u].count;
    }
    if (n_out > KZG_MAX_BATCH_OPEN)
        return fail(ctx, KZG_E_ARG, "alu: n_out, the sum of the counts, must be in [1, KZG_MAX_BATCH_OPEN]");
    BuilderCall C(ctx, "alu");
    RowTab it;
    uint32_t ki = 0;
    if (int rc = C.begin("alu", expect_i, n_input_handles, input_handles, it, &ki)) return rc;
    for (uint32_t u = 0; u < n_units; u++)
        if (units[u].op_row >= ki || units[u].a >= ki || units[u].b >= ki)
            return fail(ctx, KZG_E_ARG, "alu: a row must index the concatenated rows of the input sets");
    if (int rc = C.ready(n_out, 0, {opts ? opts->usable : 0, opts ? opts->tail_be32 : nullptr}, LAY_READ)) return rc;
    uint8_t c48[KZG_MAX_BATCH_OPEN * 48];
    uint64_t stats[4 * KZG_ALU_MAX_UNITS];
    if (int rc = rows_alu_dev(ctx, C.H, C.i, it, n_entries, program, n_units, units, n_out, C.T, C.dst(), c48, stats, C.blind))
        return rc;
    memcpy(out_commitments48, c48, 48 * (size_t)n_out);
    memcpy(out_counts, stats, 8 * (size_t)n_units);
    memcpy(out_unknown, stats + n_units, 8 * (size_t)n_units);
    memcpy(out_first, stats + 2 * n_units, 8 * (size_t)n_units);
    memcpy(out_first_unknown, stats + 3 * n_units, 8 * (size_t)n_units);
    *out_handle = C.commit();
    return KZG_OK;
}

// kzg_rows_commit_wide: a BuilderCall around its own checks.  Kinds, b, L, counts, operands, immediates and moduli are checked here, on the
// host, before a lane is taken
static bool wide_be64_zero(const uint8_t* v) {
    for (int j = 0; j < 64; j++)
        if (v[j]) return false;
    return true;
}
static bool wide_be64_fits(const uint8_t* v, uint32_t W) {   // below 2^W, W <= 512
    for (uint32_t k = W; k < 512; k++)
        if (v[63 - k / 8] >> (k % 8) & 1) return false;
    return true;
}
int rows_wide(kzg_ctx* ctx, uint32_t expect_i, uint32_t n_input_handles, const uint64_t* input_handles, uint32_t n_ops,
              const kzg_wide_op* ops, const kzg_derive_opts* opts, uint8_t* out_commitments48, uint64_t* out_counts,
              uint64_t* out_first, uint64_t* out_qover, uint64_t* out_first_qover, uint64_t* out_handle) {
    if (!ctx || !input_handles || !out_commitments48 || !out_counts || !out_first || !out_qover || !out_first_qover || !out_handle)
        return KZG_E_ARG;
    if (n_input_handles == 0 || n_input_handles > KZG_MAX_BATCH_OPEN)
        return fail(ctx, KZG_E_ARG, "wide: the number of handles must be in [1, KZG_MAX_BATCH_OPEN]");
    if (n_ops == 0 || n_ops > KZG_WIDE_MAX_OPS || !ops) return fail(ctx, KZG_E_ARG, "wide: n_ops must be in [1, KZG_WIDE_MAX_OPS]");
    uint32_t n_out = 0;
    for (uint32_t o = 0; o < n_ops; o++) {
        const kzg_wide_op& op = ops[o];
        const uint32_t L = op.limbs, W = op.bits * L;
        const bool modular = op.kind == KZG_WIDE_MULMOD || op.kind == KZG_WIDE_CARRY;
        if (op.kind < KZG_WIDE_ADD || op.kind > KZG_WIDE_CARRY)
            return fail(ctx, KZG_E_ARG, "wide: unknown kind (KZG_WIDE_ADD .. KZG_WIDE_CARRY)");
        if (op.flags & ~(KZG_WIDE_IMM_B | KZG_WIDE_NEG_C))
            return fail(ctx, KZG_E_ARG, "wide: flags must be a combination of KZG_WIDE_IMM_B and KZG_WIDE_NEG_C");
        if (op.bits == 0 || op.bits > 64) return fail(ctx, KZG_E_ARG, "wide: the limb width b must be in [1, 64]");
        if (L == 0 || L > KZG_WIDE_MAX_LIMBS) return fail(ctx, KZG_E_ARG, "wide: the number of limbs L must be in [1, 8]");
        if (W > 512) return fail(ctx, KZG_E_ARG, "wide: the width W = b L must be at most 512");
        if (op.kind == KZG_WIDE_CARRY && op.bits > 56)
            return fail(ctx, KZG_E_ARG, "wide: the limb width b of a CARRY must be at most 56");
        const bool count_ok = op.kind == KZG_WIDE_CARRY ? op.count == 2 * L - 1
                              : op.kind <= KZG_WIDE_SUB ? op.count == L || op.count == L + 1
                                                        : op.count == L || op.count == 2 * L;
        if (!count_ok)
            return fail(ctx, KZG_E_ARG, "wide: count must be L or L + 1 on ADD and SUB, L or 2 L on MUL, DIVMOD and MULMOD, 2 L - 1 on CARRY");
        if (op.a == KZG_WIDE_ABSENT) return fail(ctx, KZG_E_ARG, "wide: operand a must be given");
        if (op.flags & KZG_WIDE_IMM_B) {
            if (op.b != KZG_WIDE_ABSENT) return fail(ctx, KZG_E_ARG, "wide: operand b must be KZG_WIDE_ABSENT beside KZG_WIDE_IMM_B");
            if (!wide_be64_fits(op.imm_be64, W)) return fail(ctx, KZG_E_ARG, "wide: the immediate must be below 2^W");
        } else {
            if (!wide_be64_zero(op.imm_be64)) return fail(ctx, KZG_E_ARG, "wide: the immediate must be 0 without KZG_WIDE_IMM_B");
            if (op.b == KZG_WIDE_ABSENT && !modular)
                return fail(ctx, KZG_E_ARG, "wide: operand b must be given (a row or an immediate) on ADD, SUB, MUL and DIVMOD");
        }
        if (!modular) {
            if (op.c != KZG_WIDE_ABSENT || (op.flags & KZG_WIDE_NEG_C) || !wide_be64_zero(op.m_be64))
                return fail(ctx, KZG_E_ARG, "wide: an operand the kind does not take: c, KZG_WIDE_NEG_C and m belong to MULMOD and CARRY");
        } else {
            if (wide_be64_zero(op.m_be64)) return fail(ctx, KZG_E_ARG, "wide: the modulus m must not be 0");
            if (!wide_be64_fits(op.m_be64, W)) return fail(ctx, KZG_E_ARG, "wide: the modulus m must be below 2^W");
        }
        if (op.kind == KZG_WIDE_CARRY) {
            if (op.q == KZG_WIDE_ABSENT || op.r == KZG_WIDE_ABSENT)
                return fail(ctx, KZG_E_ARG, "wide: operands q and r must be given on CARRY");
        } else if (op.q != KZG_WIDE_ABSENT || op.r != KZG_WIDE_ABSENT) {
            return fail(ctx, KZG_E_ARG, "wide: an operand the kind does not take: q and r belong to CARRY");
        }
        n_out += op.count;
    }
    if (n_out > KZG_MAX_BATCH_OPEN)
        return fail(ctx, KZG_E_ARG, "wide: n_out, the sum of the counts, must be in [1, KZG_MAX_BATCH_OPEN]");
    BuilderCall C(ctx, "wide");
    RowTab it;
    uint32_t ki = 0;
    if (int rc = C.begin("wide", expect_i, n_input_handles, input_handles, it, &ki)) return rc;
    for (uint32_t o = 0; o < n_ops; o++)
        for (uint32_t first : {ops[o].a, ops[o].b, ops[o].c, ops[o].q, ops[o].r})
            if (first != KZG_WIDE_ABSENT && (first >= ki || ops[o].limbs > ki - first))
                return fail(ctx, KZG_E_ARG, "wide: the L rows of an operand must lie inside the concatenated rows of the input sets");
    if (int rc = C.ready(n_out, 0, {opts ? opts->usable : 0, opts ? opts->tail_be32 : nullptr}, LAY_READ)) return rc;
    uint8_t c48[KZG_MAX_BATCH_OPEN * 48];
    uint64_t stats[4 * KZG_WIDE_MAX_OPS];
    if (int rc = rows_wide_dev(ctx, C.H, C.i, it, n_ops, ops, n_out, C.T, C.dst(), c48, stats, C.blind)) return rc;
    memcpy(out_commitments48, c48, 48 * (size_t)n_out);
    memcpy(out_counts, stats, 8 * (size_t)n_ops);
    memcpy(out_qover, stats + n_ops, 8 * (size_t)n_ops);
    memcpy(out_first, stats + 2 * n_ops, 8 * (size_t)n_ops);
    memcpy(out_first_qover, stats + 3 * n_ops, 8 * (size_t)n_ops);
    *out_handle = C.commit();
    return KZG_OK;
}

// The ranges of R_F and R_P in the words of every Poseidon parameter check: the refusal, or null
static const char* poseidon_rounds_why(uint32_t full, uint32_t partial) {
    if (full < 2 || full > KZG_POSEIDON_MAX_FULL || (full & 1)) return "the number of full rounds R_F must be even and in [2, 16]";
    if (partial > KZG_POSEIDON_MAX_PARTIAL) return "the number of partial rounds R_P must be in [0, 128]";
    return nullptr;
}
// The checks of kzg_poseidon_params, shared by kzg_rows_commit_poseidon and kzg_rows_commit_poseidon_chain (`what` prefixes the
// messages): the ranges of t, R_F and R_P, then the number of units (units_ok, with the words of its refusal), then every
// constant and matrix entry canonical
static int poseidon_params_check(kzg_ctx* ctx, const char* what, const kzg_poseidon_params* params, bool units_ok,
                                 const char* units_why) {
    auto bad = [&](const char* why) { return fail(ctx, KZG_E_ARG, std::string(what) + ": " + why); };
    if (!params || !params->rc_be32 || !params->mds_be32) return bad("params, rc_be32 and mds_be32 must not be null");
    const uint32_t t = params->t, R = params->full + params->partial;
    if (t < KZG_POSEIDON_MIN_T || t > KZG_POSEIDON_MAX_T) return bad("the width t must be in [2, 8]");
    if (const char* why = poseidon_rounds_why(params->full, params->partial)) return bad(why);
    if (!units_ok) return bad(units_why);
    for (uint32_t k = 0; k < t * R; k++)
        if (!fr_be32_canonical(params->rc_be32 + 32 * (size_t)k)) return bad("round constants must be canonical scalars (< r)");
    for (uint32_t k = 0; k < t * t; k++)
        if (!fr_be32_canonical(params->mds_be32 + 32 * (size_t)k)) return bad("matrix entries must be canonical scalars (< r)");
    return KZG_OK;
}
// The checks of kzg_poseidon2_params, in the same order: t, R_F and R_P, the number of units, every constant canonical
static int poseidon2_params_check(kzg_ctx* ctx, const kzg_poseidon2_params* params, bool units_ok) {
    auto bad = [&](const char* why) { return fail(ctx, KZG_E_ARG, std::string("poseidon2: ") + why); };
    if (!params || !params->rc_full_be32 || !params->diag_be32 || (params->partial && !params->rc_partial_be32))
        return bad("params, rc_full_be32, rc_partial_be32 (with R_P > 0) and diag_be32 must not be null");
    const uint32_t t = params->t;
    if (t >= 32 || !(KZG_POSEIDON2_WIDTHS >> t & 1)) return bad("the width t must be 2, 3, 4 or 8");
    if (const char* why = poseidon_rounds_why(params->full, params->partial)) return bad(why);
    if (!units_ok) return bad("n_units must be in [1, KZG_POSEIDON2_MAX_UNITS]");
    for (uint32_t k = 0; k < t * params->full; k++)
        if (!fr_be32_canonical(params->rc_full_be32 + 32 * (size_t)k)) return bad("round constants must be canonical scalars (< r)");
    for (uint32_t k = 0; k < params->partial; k++)
        if (!fr_be32_canonical(params->rc_partial_be32 + 32 * (size_t)k)) return bad("round constants must be canonical scalars (< r)");
    for (uint32_t k = 0; k < t; k++)
        if (!fr_be32_canonical(params->diag_be32 + 32 * (size_t)k)) return bad("diagonal entries must be canonical scalars (< r)");
    return KZG_OK;
}

// The units of kzg_rows_commit_poseidon and kzg_rows_commit_poseidon2 (one struct, one meaning), behind the parameter checks:
// modes, flags, periods (a trace block holds R + lead rows: lead = 1 for Poseidon, 2 for Poseidon2 with its row of E(input)), out
// lists, immediates and the two caps; then the UnitCall, the builder's device call `dev`, the statistics and the new set.
// `what` prefixes the messages
template <class Dev>
static int rows_poseidon_units(kzg_ctx* ctx, const char* what, uint32_t t, uint32_t R, uint32_t lead, uint32_t expect_i,
                               uint32_t n_input_handles, const uint64_t* input_handles, uint32_t n_units,
                               const kzg_poseidon_unit* units, const kzg_derive_opts* opts, uint8_t* out_commitments48,
                               uint64_t* out_perms, uint64_t* out_mismatch, uint64_t* out_first_mismatch, uint64_t* out_handle,
                               Dev dev) {
    auto bad = [&](const std::string& why) { return fail(ctx, KZG_E_ARG, std::string(what) + ": " + why); };
    uint32_t n_out = 0;
    SeenRows S;
    for (uint32_t u = 0; u < n_units; u++) {
        const kzg_poseidon_unit& U = units[u];
        if (U.mode != KZG_POSEIDON_ROW && U.mode != KZG_POSEIDON_ROUNDS)
            return bad("unknown mode (KZG_POSEIDON_ROW or KZG_POSEIDON_ROUNDS)");
        if (U.flags & ~KZG_POSEIDON_CHECK) return bad("flags must be 0 or KZG_POSEIDON_CHECK");
        const bool rounds = U.mode == KZG_POSEIDON_ROUNDS, check = U.flags == KZG_POSEIDON_CHECK;
        if (rounds && check) return bad("expect (KZG_POSEIDON_CHECK) belongs to ROW units, not to ROUNDS");
        if (rounds ? U.period < R + lead : U.period != 0)
            return bad("the period P of a ROUNDS unit must be at least R + " + std::to_string(lead) + " (0 on a ROW unit)");
        if (rounds ? U.n_out != t : (U.n_out == 0 || U.n_out > t))
            return bad("n_out must be in [1, t] on a ROW unit and t on a ROUNDS unit");
        uint32_t taken = 0;
        for (uint32_t c = 0; c < U.n_out; c++) {
            if (U.out[c] >= t || (rounds && U.out[c] != c)) return bad("an out index must be below t (ROUNDS: out[j] = j)");
            if (taken >> U.out[c] & 1) return bad("an out index is repeated");
            taken |= 1u << U.out[c];
            if (check) S.see(U.expect[c]);
        }
        for (uint32_t j = 0; j < t; j++) {
            if (U.in[j] != KZG_POSEIDON_IMM) {
                S.see(U.in[j]);
                for (int b = 0; b < 32; b++)
                    if (U.imm_be32[j][b]) return bad("the immediate must be 0 beside a row");
            } else if (!fr_be32_canonical(U.imm_be32[j])) {
                return bad("immediates must be canonical scalars (< r)");
            }
        }
        if (S.too_many()) return bad("a call reads at most KZG_MAX_BATCH_OPEN distinct input rows");
        n_out += check ? 0 : U.n_out;
    }
    if (n_out > KZG_MAX_BATCH_OPEN) return bad("n_out, the committed columns of all units, must be at most KZG_MAX_BATCH_OPEN");
    if (n_out && !out_commitments48) return KZG_E_ARG;
    UnitCall C(ctx, what);
    if (int rc = C.open(expect_i, n_input_handles, input_handles, S.n != 0, S.max_row, ROW_WHY, n_out, opts)) return rc;
    uint64_t stats[2 * KZG_POSEIDON_MAX_UNITS];
    if (int rc = dev(C, n_out, stats)) return rc;
    const uint64_t n = C.n_read();
    for (uint32_t u = 0; u < n_units; u++) out_perms[u] = units[u].mode == KZG_POSEIDON_ROUNDS ? n / units[u].period : n;
    static const int run_of[3] = {-1, 0, 1};   // the device's runs: mismatches, then their first rows
    uint64_t* const out[3] = {out_perms, out_mismatch, out_first_mismatch};
    stats_scatter(out, run_of, 3, stats, n_units);
    C.finish(out_commitments48, out_handle);
    return KZG_OK;
}

// kzg_rows_commit_poseidon: a BuilderCall around its own checks; as in rows_expr, no reservation and no set when every unit is
// a check.  The parameters, the constants and immediates, modes, flags and out lists are checked here, on the host, before a
// lane is taken
int rows_poseidon(kzg_ctx* ctx, uint32_t expect_i, uint32_t n_input_handles, const uint64_t* input_handles,
                  const kzg_poseidon_params* params, uint32_t n_units, const kzg_poseidon_unit* units, const kzg_derive_opts* opts,
                  uint8_t* out_commitments48, uint64_t* out_perms, uint64_t* out_mismatch, uint64_t* out_first_mismatch,
                  uint64_t* out_handle) {
    if (!ctx || !input_handles || !out_perms || !out_mismatch || !out_first_mismatch || !out_handle) return KZG_E_ARG;
    if (int rc = UnitCall::handles_ok(ctx, "poseidon", n_input_handles)) return rc;
    if (int rc = poseidon_params_check(ctx, "poseidon", params, n_units != 0 && n_units <= KZG_POSEIDON_MAX_UNITS && units,
                                       "n_units must be in [1, KZG_POSEIDON_MAX_UNITS]"))
        return rc;
    return rows_poseidon_units(ctx, "poseidon", params->t, params->full + params->partial, 1, expect_i, n_input_handles,
                               input_handles, n_units, units, opts, out_commitments48, out_perms, out_mismatch,
                               out_first_mismatch, out_handle, [&](UnitCall& C, uint32_t n_out, uint64_t* stats) {
                                   return rows_poseidon_dev(ctx, C.H, C.i, C.it, params, n_units, units, n_out, C.T, C.dst(),
                                                            C.c48, stats, C.blind);
                               });
}

// kzg_rows_commit_poseidon2: rows_poseidon with its own parameters and device call; a trace block has one row more
int rows_poseidon2(kzg_ctx* ctx, uint32_t expect_i, uint32_t n_input_handles, const uint64_t* input_handles,
                   const kzg_poseidon2_params* params, uint32_t n_units, const kzg_poseidon_unit* units,
                   const kzg_derive_opts* opts, uint8_t* out_commitments48, uint64_t* out_perms, uint64_t* out_mismatch,
                   uint64_t* out_first_mismatch, uint64_t* out_handle) {
    if (!ctx || !input_handles || !out_perms || !out_mismatch || !out_first_mismatch || !out_handle) return KZG_E_ARG;
    if (int rc = UnitCall::handles_ok(ctx, "poseidon2", n_input_handles)) return rc;
    if (int rc = poseidon2_params_check(ctx, params, n_units != 0 && n_units <= KZG_POSEIDON2_MAX_UNITS && units)) return rc;
    return rows_poseidon_units(ctx, "poseidon2", params->t, params->full + params->partial, 2, expect_i, n_input_handles,
                               input_handles, n_units, units, opts, out_commitments48, out_perms, out_mismatch,
                               out_first_mismatch, out_handle, [&](UnitCall& C, uint32_t n_out, uint64_t* stats) {
                                   return rows_poseidon2_dev(ctx, C.H, C.i, C.it, params, n_units, units, n_out, C.T, C.dst(),
                                                             C.c48, stats, C.blind);
                               });
}

// kzg_rows_commit_poseidon_chain: a BuilderCall around its own checks; as in rows_poseidon, no reservation and no set when every
// unit is a check.  The parameters, modes, flags, layouts, periods, column ids and the entries a mode does not take are checked
// here, on the host, before a lane is taken
int rows_poseidon_chain(kzg_ctx* ctx, uint32_t expect_i, uint32_t n_input_handles, const uint64_t* input_handles,
                        const kzg_poseidon_params* params, uint32_t n_units, const kzg_poseidon_chain_unit* units,
                        const kzg_derive_opts* opts, uint8_t* out_commitments48, uint64_t* const out_stats[6], uint64_t* out_handle) {
    if (!ctx || !input_handles || !out_stats || !out_handle) return KZG_E_ARG;
    for (int k = 0; k < 6; k++)
        if (!out_stats[k]) return KZG_E_ARG;
    auto bad = [&](const char* why) { return fail(ctx, KZG_E_ARG, std::string("poseidon_chain: ") + why); };
    if (int rc = UnitCall::handles_ok(ctx, "poseidon_chain", n_input_handles)) return rc;
    if (int rc = poseidon_params_check(ctx, "poseidon_chain", params, n_units != 0 && n_units <= KZG_POSEIDON_CHAIN_MAX_UNITS && units,
                                       "n_units must be in [1, KZG_POSEIDON_CHAIN_MAX_UNITS]"))
        return rc;
    const uint32_t t = params->t, R = params->full + params->partial, ABSENT = KZG_POSEIDON_CHAIN_ABSENT;
    uint32_t n_out = 0;
    SeenRows S;
    for (uint32_t u = 0; u < n_units; u++) {
        const kzg_poseidon_chain_unit& U = units[u];
        if (U.mode != KZG_POSEIDON_CHAIN_SPONGE && U.mode != KZG_POSEIDON_CHAIN_PATH)
            return bad("unknown mode (KZG_POSEIDON_CHAIN_SPONGE or KZG_POSEIDON_CHAIN_PATH)");
        if ((U.flags & ~KZG_POSEIDON_CHAIN_CHECK) || U.reserved) return bad("flags must be 0 or KZG_POSEIDON_CHAIN_CHECK, reserved 0");
        const bool path = U.mode == KZG_POSEIDON_CHAIN_PATH, check = U.flags == KZG_POSEIDON_CHAIN_CHECK;
        if (path && t < 3) return bad("a PATH unit needs t >= 3 (the arity is t - 1)");
        if (U.period == 0) return bad("the period P must be in [1, 2^32)");
        if (check) {
            if (U.layout || U.n_out) return bad("layout and n_out must be 0 beside KZG_POSEIDON_CHAIN_CHECK: a check commits nothing");
            if (U.expect == ABSENT) return bad("expect must be a row with KZG_POSEIDON_CHAIN_CHECK, not an immediate or absent");
            S.see(U.expect);
        } else {
            if (U.expect != ABSENT) return bad("expect belongs to KZG_POSEIDON_CHAIN_CHECK (KZG_POSEIDON_CHAIN_ABSENT without)");
            if (U.layout != KZG_POSEIDON_CHAIN_TRACE && U.layout != KZG_POSEIDON_CHAIN_FLAT)
                return bad("unknown layout (KZG_POSEIDON_CHAIN_TRACE or KZG_POSEIDON_CHAIN_FLAT)");
            const bool trace = U.layout == KZG_POSEIDON_CHAIN_TRACE;
            if (trace && U.period <= R) return bad("the period P of a TRACE unit must be at least R + 1");
            if (trace ? U.n_out != t : (U.n_out == 0 || U.n_out > 2 * t))
                return bad("n_out must be t on a TRACE unit and in [1, 2 t] on a FLAT unit");
            uint32_t taken = 0;
            for (uint32_t c = 0; c < U.n_out; c++) {
                const uint32_t id = U.out[c];
                if (trace ? id != c : (id % KZG_POSEIDON_CHAIN_COL_OUT >= t || id >= 2 * KZG_POSEIDON_CHAIN_COL_OUT))
                    return bad("unknown column id (TRACE: out[j] = j; FLAT: KZG_POSEIDON_CHAIN_COL_IN / _OUT + j, j < t)");
                if (taken >> id & 1) return bad("a column id is repeated");
                taken |= 1u << id;
            }
        }
        if (path || check) {
            if (U.digest >= t) return bad("digest must be a state index below t on a PATH unit and on a check");
        } else if (U.digest != ABSENT) {
            return bad("digest belongs to PATH units and checks (KZG_POSEIDON_CHAIN_ABSENT elsewhere)");
        }
        if (path) {
            if (U.pos == ABSENT) return bad("pos must be a row on a PATH unit, not an immediate or absent");
            S.see(U.pos);
        } else if (U.pos != ABSENT) {
            return bad("pos belongs to PATH units (KZG_POSEIDON_CHAIN_ABSENT on a SPONGE unit)");
        }
        if (U.start != ABSENT) S.see(U.start);
        for (uint32_t j = 0; j < KZG_POSEIDON_MAX_T; j++) {
            if (j >= t) {
                bool zero = U.in[j] == 0;
                for (int b = 0; b < 32; b++) zero = zero && !U.imm_be32[j][b];
                if (!zero) return bad("the entries of in and imm_be32 at and above t must be 0");
            } else if (U.in[j] != KZG_POSEIDON_IMM) {
                S.see(U.in[j]);
                for (int b = 0; b < 32; b++)
                    if (U.imm_be32[j][b]) return bad("the immediate must be 0 beside a row");
            } else if (path && j >= 2) {
                return bad("a sibling of a PATH unit is a row, not an immediate");
            } else if (!fr_be32_canonical(U.imm_be32[j])) {
                return bad("immediates must be canonical scalars (< r)");
            }
        }
        if (S.too_many()) return bad("a call reads at most KZG_MAX_BATCH_OPEN distinct input rows");
        n_out += U.n_out;
    }
    if (n_out > KZG_MAX_BATCH_OPEN) return bad("n_out, the committed columns of all units, must be at most KZG_MAX_BATCH_OPEN");
    if (n_out && !out_commitments48) return KZG_E_ARG;
    UnitCall C(ctx, "poseidon_chain");
    if (int rc = C.open(expect_i, n_input_handles, input_handles, S.n != 0, S.max_row, ROW_WHY, n_out, opts)) return rc;
    uint64_t stats[5 * KZG_POSEIDON_CHAIN_MAX_UNITS];
    if (int rc = rows_poseidon_chain_dev(ctx, C.H, C.i, C.it, params, n_units, units, n_out, C.T, C.dst(), C.c48, stats, C.blind))
        return rc;
    const uint64_t n = C.n_read();
    for (uint32_t u = 0; u < n_units; u++) out_stats[0][u] = n / units[u].period;
    // the device's runs: segments, bad positions, mismatches, then the first rows of the last two
    static const int run_of[6] = {-1, 0, 1, 3, 2, 4};
    stats_scatter(out_stats, run_of, 6, stats, n_units);
    C.finish(out_commitments48, out_handle);
    return KZG_OK;
}

// kzg_rows_commit_sha256: a BuilderCall around its own checks; as in rows_poseidon, no reservation and no set when every unit is
// a check.  Modes, flags, periods, out lists and the entries a mode does not take are checked here, on the host, before a lane
// is taken
int rows_sha256(kzg_ctx* ctx, uint32_t expect_i, uint32_t n_input_handles, const uint64_t* input_handles, uint32_t n_units,
                const kzg_sha256_unit* units, const kzg_derive_opts* opts, uint8_t* out_commitments48, uint64_t* out_blocks,
                uint64_t* out_messages, uint64_t* out_counts, uint64_t* out_first, uint64_t* out_mismatch,
                uint64_t* out_first_mismatch, uint64_t* out_handle) {
    if (!ctx || !input_handles || !out_blocks || !out_messages || !out_counts || !out_first || !out_mismatch ||
        !out_first_mismatch || !out_handle)
        return KZG_E_ARG;
    if (int rc = UnitCall::handles_ok(ctx, "sha256", n_input_handles)) return rc;
    if (n_units == 0 || n_units > KZG_SHA256_MAX_UNITS || !units)
        return fail(ctx, KZG_E_ARG, "sha256: n_units must be in [1, KZG_SHA256_MAX_UNITS]");
    uint32_t n_out = 0;
    SeenRows S;
    for (uint32_t u = 0; u < n_units; u++) {
        const kzg_sha256_unit& U = units[u];
        if (U.mode != KZG_SHA256_ROW && U.mode != KZG_SHA256_ROUNDS)
            return fail(ctx, KZG_E_ARG, "sha256: unknown mode (KZG_SHA256_ROW or KZG_SHA256_ROUNDS)");
        if (U.flags & ~(KZG_SHA256_CHECK | KZG_SHA256_STD_IV))
            return fail(ctx, KZG_E_ARG, "sha256: flags must be a combination of KZG_SHA256_CHECK and KZG_SHA256_STD_IV");
        const bool rounds = U.mode == KZG_SHA256_ROUNDS, check = U.flags & KZG_SHA256_CHECK, std_iv = U.flags & KZG_SHA256_STD_IV;
        if (rounds && check) return fail(ctx, KZG_E_ARG, "sha256: expect (KZG_SHA256_CHECK) belongs to ROW units, not to ROUNDS");
        if (rounds ? U.period < KZG_SHA256_MIN_PERIOD : U.period != 0)
            return fail(ctx, KZG_E_ARG, "sha256: the period P of a ROUNDS unit must be at least 72 (0 on a ROW unit)");
        const uint32_t top = rounds ? KZG_SHA256_N_COLS : 8;
        if (U.n_out == 0 || U.n_out > top)
            return fail(ctx, KZG_E_ARG, "sha256: n_out must be in [1, 8] on a ROW unit and in [1, 12] on a ROUNDS unit");
        uint32_t taken = 0;
        for (uint32_t c = 0; c < U.n_out; c++) {
            if (U.out[c] >= top)
                return fail(ctx, KZG_E_ARG, "sha256: an out index must be below 8 (ROUNDS: a column id below KZG_SHA256_N_COLS)");
            if (taken >> U.out[c] & 1) return fail(ctx, KZG_E_ARG, "sha256: an out index is repeated");
            taken |= 1u << U.out[c];
            if (check) S.see(U.expect[c]);
        }
        for (uint32_t j = 0; j < 8; j++) {
            if (U.state[j] != KZG_SHA256_IMM) {
                if (rounds || std_iv)
                    return fail(ctx, KZG_E_ARG, "sha256: a state entry must be KZG_SHA256_IMM on a ROUNDS unit and with KZG_SHA256_STD_IV");
                if (U.state_imm[j]) return fail(ctx, KZG_E_ARG, "sha256: the immediate must be 0 beside a row");
                S.see(U.state[j]);
            } else if (std_iv && U.state_imm[j]) {
                return fail(ctx, KZG_E_ARG, "sha256: the immediate must be 0 with KZG_SHA256_STD_IV");
            }
        }
        for (uint32_t j = 0; j < 16; j++) {
            if (rounds) {
                if (j == 0 && U.msg[0] == KZG_SHA256_IMM)
                    return fail(ctx, KZG_E_ARG, "sha256: the message of a ROUNDS unit is a row, not an immediate");
                if ((j && U.msg[j]) || U.msg_imm[j])
                    return fail(ctx, KZG_E_ARG, "sha256: msg[1 .. 15] and msg_imm must be 0 on a ROUNDS unit");
                if (j == 0) S.see(U.msg[0]);
            } else if (U.msg[j] != KZG_SHA256_IMM) {
                if (U.msg_imm[j]) return fail(ctx, KZG_E_ARG, "sha256: the immediate must be 0 beside a row");
                S.see(U.msg[j]);
            }
        }
        if (U.start != KZG_SHA256_ABSENT) {
            if (!rounds) return fail(ctx, KZG_E_ARG, "sha256: start belongs to ROUNDS units (KZG_SHA256_ABSENT on a ROW unit)");
            S.see(U.start);
        }
        if (S.too_many())
            return fail(ctx, KZG_E_ARG, "sha256: a call reads at most KZG_MAX_BATCH_OPEN distinct input rows");
        n_out += check ? 0 : U.n_out;
    }
    if (n_out > KZG_MAX_BATCH_OPEN)
        return fail(ctx, KZG_E_ARG, "sha256: n_out, the committed columns of all units, must be at most KZG_MAX_BATCH_OPEN");
    if (n_out && !out_commitments48) return KZG_E_ARG;
    UnitCall C(ctx, "sha256");
    if (int rc = C.open(expect_i, n_input_handles, input_handles, S.n != 0, S.max_row, ROW_WHY, n_out, opts)) return rc;
    uint64_t stats[5 * KZG_SHA256_MAX_UNITS];
    if (int rc = rows_sha256_dev(ctx, C.H, C.i, C.it, n_units, units, n_out, C.T, C.dst(), C.c48, stats, C.blind)) return rc;
    const uint64_t n = C.n_read();
    for (uint32_t u = 0; u < n_units; u++) out_blocks[u] = units[u].mode == KZG_SHA256_ROUNDS ? n / units[u].period : n;
    static const int run_of[6] = {-1, 2, 0, 3, 1, 4};   // the device's runs: counts, mismatches, messages, then two first rows
    uint64_t* const out[6] = {out_blocks, out_messages, out_counts, out_first, out_mismatch, out_first_mismatch};
    stats_scatter(out, run_of, 6, stats, n_units);
    C.finish(out_commitments48, out_handle);
    return KZG_OK;
}

// kzg_rows_commit_keccak: a BuilderCall around its own checks; as in rows_sha256, no reservation and no set when every unit is a
// check.  Modes, flags, periods, rates, out lists and the entries a mode does not take are checked here, on the host, before a
// lane is taken
int rows_keccak(kzg_ctx* ctx, uint32_t expect_i, uint32_t n_input_handles, const uint64_t* input_handles, uint32_t n_units,
                const kzg_keccak_unit* units, const kzg_derive_opts* opts, uint8_t* out_commitments48, uint64_t* out_perms,
                uint64_t* out_messages, uint64_t* out_counts, uint64_t* out_first, uint64_t* out_mismatch,
                uint64_t* out_first_mismatch, uint64_t* out_handle) {
    if (!ctx || !input_handles || !out_perms || !out_messages || !out_counts || !out_first || !out_mismatch ||
        !out_first_mismatch || !out_handle)
        return KZG_E_ARG;
    if (int rc = UnitCall::handles_ok(ctx, "keccak", n_input_handles)) return rc;
    if (n_units == 0 || n_units > KZG_KECCAK_MAX_UNITS || !units)
        return fail(ctx, KZG_E_ARG, "keccak: n_units must be in [1, KZG_KECCAK_MAX_UNITS]");
    uint32_t n_out = 0;
    SeenRows S;
    for (uint32_t u = 0; u < n_units; u++) {
        const kzg_keccak_unit& U = units[u];
        if (U.mode != KZG_KECCAK_ROW && U.mode != KZG_KECCAK_ROUNDS)
            return fail(ctx, KZG_E_ARG, "keccak: unknown mode (KZG_KECCAK_ROW or KZG_KECCAK_ROUNDS)");
        if (U.flags & ~KZG_KECCAK_CHECK) return fail(ctx, KZG_E_ARG, "keccak: flags must be 0 or KZG_KECCAK_CHECK");
        const bool rounds = U.mode == KZG_KECCAK_ROUNDS, check = U.flags & KZG_KECCAK_CHECK;
        if (rounds && check) return fail(ctx, KZG_E_ARG, "keccak: expect (KZG_KECCAK_CHECK) belongs to ROW units, not to ROUNDS");
        if (rounds ? U.period < KZG_KECCAK_MIN_PERIOD : U.period != 0)
            return fail(ctx, KZG_E_ARG, "keccak: the period P of a ROUNDS unit must be at least 125 (0 on a ROW unit)");
        if (rounds ? U.rate == 0 || U.rate > 24 : U.rate != 0)
            return fail(ctx, KZG_E_ARG, "keccak: the rate of a ROUNDS unit must be in [1, 24] lanes (0 on a ROW unit)");
        if (U.n_out == 0 || U.n_out > KZG_KECCAK_MAX_OUT)
            return fail(ctx, KZG_E_ARG, "keccak: n_out must be in [1, KZG_KECCAK_MAX_OUT]");
        uint32_t taken = 0;
        for (uint32_t c = 0; c < U.n_out; c++) {
            if (U.out[c] >= KZG_KECCAK_N_COLS)
                return fail(ctx, KZG_E_ARG, "keccak: a lane index must be below 25 (ROUNDS: a column id below KZG_KECCAK_N_COLS)");
            if (taken >> U.out[c] & 1) return fail(ctx, KZG_E_ARG, "keccak: a lane index or column id is repeated");
            taken |= 1u << U.out[c];
            if (check) S.see(U.expect[c]);
        }
        for (uint32_t j = 0; j < 25; j++) {
            if (rounds) {
                if (j < 5 && U.in[j] == KZG_KECCAK_IMM)
                    return fail(ctx, KZG_E_ARG, "keccak: the message columns of a ROUNDS unit are rows, not immediates");
                if ((j >= 5 && U.in[j]) || U.imm[j])
                    return fail(ctx, KZG_E_ARG, "keccak: in[5 .. 24] and imm must be 0 on a ROUNDS unit");
                if (j < 5) S.see(U.in[j]);
            } else if (U.in[j] != KZG_KECCAK_IMM) {
                if (U.imm[j]) return fail(ctx, KZG_E_ARG, "keccak: the immediate must be 0 beside a row");
                S.see(U.in[j]);
            }
        }
        if (U.start != KZG_KECCAK_ABSENT) {
            if (!rounds) return fail(ctx, KZG_E_ARG, "keccak: start belongs to ROUNDS units (KZG_KECCAK_ABSENT on a ROW unit)");
            S.see(U.start);
        }
        if (S.too_many())
            return fail(ctx, KZG_E_ARG, "keccak: a call reads at most KZG_MAX_BATCH_OPEN distinct input rows");
        n_out += check ? 0 : U.n_out;
    }
    if (n_out > KZG_MAX_BATCH_OPEN)
        return fail(ctx, KZG_E_ARG, "keccak: n_out, the committed columns of all units, must be at most KZG_MAX_BATCH_OPEN");
    if (n_out && !out_commitments48) return KZG_E_ARG;
    UnitCall C(ctx, "keccak");
    if (int rc = C.open(expect_i, n_input_handles, input_handles, S.n != 0, S.max_row, ROW_WHY, n_out, opts)) return rc;
    uint64_t stats[5 * KZG_KECCAK_MAX_UNITS];
    if (int rc = rows_keccak_dev(ctx, C.H, C.i, C.it, n_units, units, n_out, C.T, C.dst(), C.c48, stats, C.blind)) return rc;
    const uint64_t n = C.n_read();
    for (uint32_t u = 0; u < n_units; u++) out_perms[u] = units[u].mode == KZG_KECCAK_ROUNDS ? n / units[u].period : n;
    static const int run_of[6] = {-1, 2, 0, 3, 1, 4};   // the device's runs: counts, mismatches, messages, then two first rows
    uint64_t* const out[6] = {out_perms, out_messages, out_counts, out_first, out_mismatch, out_first_mismatch};
    stats_scatter(out, run_of, 6, stats, n_units);
    C.finish(out_commitments48, out_handle);
    return KZG_OK;
}

// kzg_rows_commit_ec: a BuilderCall around its own checks; as in rows_keccak, no reservation and no set when every unit is a
// check.  The curve, modes, flags, names and the entries a mode does not take are checked here, on the host, before a lane is
// taken
int rows_ec(kzg_ctx* ctx, uint32_t expect_i, uint32_t n_input_handles, const uint64_t* input_handles, const kzg_ec_curve* curve,
            uint32_t n_units, const kzg_ec_unit* units, const kzg_derive_opts* opts, uint8_t* out_commitments48,
            uint64_t* const out_stats[9], uint64_t* out_handle) {
    if (!ctx || !input_handles || !out_stats || !out_handle) return KZG_E_ARG;
    for (int k = 0; k < 9; k++)
        if (!out_stats[k]) return KZG_E_ARG;
    if (int rc = UnitCall::handles_ok(ctx, "ec", n_input_handles)) return rc;
    if (n_units == 0 || n_units > KZG_EC_MAX_UNITS || !units)
        return fail(ctx, KZG_E_ARG, "ec: n_units must be in [1, KZG_EC_MAX_UNITS]");
    if (!curve) return fail(ctx, KZG_E_ARG, "ec: the curve must be given");
    const uint32_t b = curve->bits, L = curve->limbs;
    if (b == 0 || b > 64) return fail(ctx, KZG_E_ARG, "ec: the limb width b (bits) must be in [1, 64]");
    if (L == 0 || L > KZG_EC_MAX_LIMBS) return fail(ctx, KZG_E_ARG, "ec: the number of limbs L (limbs) must be in [1, KZG_EC_MAX_LIMBS]");
    const uint32_t W = b * L;
    if (W > 256) return fail(ctx, KZG_E_ARG, "ec: the width W = b L must be at most 256");
    // x < 2^W; x < y; as little-endian words
    auto fits = [&](const uint64_t* x) {
        for (uint32_t w = 0; w < 4; w++) {
            const uint32_t lo = 64 * w;
            if (lo >= W ? x[w] != 0 : (W - lo < 64 && (x[w] >> (W - lo)) != 0)) return false;
        }
        return true;
    };
    auto below = [](const uint64_t* x, const uint64_t* y) {
        for (int w = 3; w >= 0; w--)
            if (x[w] != y[w]) return x[w] < y[w];
        return false;
    };
    const bool p_small = !curve->p[1] && !curve->p[2] && !curve->p[3] && curve->p[0] < 3;
    if (!(curve->p[0] & 1u) || p_small) return fail(ctx, KZG_E_ARG, "ec: the modulus p must be odd and at least 3");
    if (!fits(curve->p)) return fail(ctx, KZG_E_ARG, "ec: the modulus p must be below 2^W");
    if (!below(curve->a, curve->p)) return fail(ctx, KZG_E_ARG, "ec: the coefficient a must be below p");
    uint32_t n_out = 0;
    SeenRows S;
    for (uint32_t u = 0; u < n_units; u++) {
        const kzg_ec_unit& U = units[u];
        if (U.mode != KZG_EC_DIV && U.mode != KZG_EC_ADD && U.mode != KZG_EC_CHAIN)
            return fail(ctx, KZG_E_ARG, "ec: unknown mode (KZG_EC_DIV, KZG_EC_ADD or KZG_EC_CHAIN)");
        if (U.flags & ~(KZG_EC_CHECK | KZG_EC_IMM_B) || U.reserved)
            return fail(ctx, KZG_E_ARG, "ec: flags must be made of KZG_EC_CHECK and KZG_EC_IMM_B, reserved must be 0");
        const bool check = U.flags & KZG_EC_CHECK, imm_b = U.flags & KZG_EC_IMM_B;
        if (check && U.mode == KZG_EC_CHAIN) return fail(ctx, KZG_E_ARG, "ec: expect (KZG_EC_CHECK) belongs to DIV and ADD units, not to CHAIN");
        if (imm_b && U.mode != KZG_EC_DIV) return fail(ctx, KZG_E_ARG, "ec: an immediate (KZG_EC_IMM_B) belongs to DIV units");
        const uint32_t names = U.mode == KZG_EC_DIV ? KZG_EC_R : 7u, n_in = U.mode == KZG_EC_ADD ? 4u : 2u;
        if (!U.cols || (U.cols & ~names)) return fail(ctx, KZG_E_ARG, "ec: cols must name at least one column, and only columns of the unit's mode");
        for (uint32_t w = 0; w < 4; w++) {
            const bool takes = w < n_in && !(w == 1 && imm_b);
            if (takes != (U.in[w] != KZG_EC_ABSENT))
                return fail(ctx, KZG_E_ARG, "ec: an operand the mode does not take, or a missing one (KZG_EC_ABSENT beside the mode's operands)");
            if (takes) S.see_run(U.in[w], L);
            if (!imm_b && U.imm[w]) return fail(ctx, KZG_E_ARG, "ec: the immediate must be 0 without KZG_EC_IMM_B");
        }
        if (imm_b && !fits(U.imm)) return fail(ctx, KZG_E_ARG, "ec: the immediate must be below 2^W");
        if ((U.mode == KZG_EC_CHAIN) != (U.op != KZG_EC_ABSENT))
            return fail(ctx, KZG_E_ARG, "ec: op belongs to CHAIN units, and a CHAIN unit must have one (KZG_EC_ABSENT elsewhere)");
        if (U.mode == KZG_EC_CHAIN) S.see_run(U.op, 1);
        for (uint32_t k = 0; k < 3; k++) {
            const bool takes = check && (U.cols >> k & 1u);
            if (takes != (U.expect[k] != KZG_EC_ABSENT))
                return fail(ctx, KZG_E_ARG, "ec: expect must hold one first row per name of cols under KZG_EC_CHECK, KZG_EC_ABSENT elsewhere");
            if (takes) S.see_run(U.expect[k], L);
        }
        if (S.too_many())
            return fail(ctx, KZG_E_ARG, "ec: a call reads at most KZG_MAX_BATCH_OPEN distinct input rows");
        n_out += check ? 0 : (uint32_t)__builtin_popcount(U.cols) * L;
    }
    if (n_out > KZG_MAX_BATCH_OPEN)
        return fail(ctx, KZG_E_ARG, "ec: n_out, the committed rows of all units, must be at most KZG_MAX_BATCH_OPEN");
    if (n_out && !out_commitments48) return KZG_E_ARG;
    UnitCall C(ctx, "ec");
    // (no guard on S.n: every unit of ec names a row)
    static const char run_why[] = ": an operand run must lie inside the concatenated rows of the input sets";
    if (int rc = C.open(expect_i, n_input_handles, input_handles, true, S.max_row, run_why, n_out, opts)) return rc;
    uint64_t stats[7 * KZG_EC_MAX_UNITS];
    if (int rc = rows_ec_dev(ctx, C.H, C.i, C.it, curve, n_units, units, n_out, C.T, C.dst(), C.c48, stats, C.blind)) return rc;
    // the device's runs: counts, singular, mismatch or unknown, segments, first, first_singular, first of the third
    static const int run_of[9] = {0, 4, 1, 5, -1, -1, -1, -1, 3};
    bool chain[KZG_EC_MAX_UNITS];
    for (uint32_t u = 0; u < n_units; u++) chain[u] = units[u].mode == KZG_EC_CHAIN;
    stats_scatter(out_stats, run_of, 9, stats, n_units);
    stats_split(out_stats, 2, 4, 6, 0, stats, n_units, chain);
    stats_split(out_stats, 6, 5, 7, KZG_EC_NONE, stats, n_units, chain);
    C.finish(out_commitments48, out_handle);
    return KZG_OK;
}

// kzg_rows_commit_edwards: a BuilderCall around its own checks; as in rows_ec, no reservation and no set when every unit is a
// check.  The curve, the immediates, modes, flags, names, out orders and the entries a mode does not take are checked here, on
// the host, before a lane is taken
int rows_edwards(kzg_ctx* ctx, uint32_t expect_i, uint32_t n_input_handles, const uint64_t* input_handles,
                 const kzg_edwards_curve* curve, uint32_t n_units, const kzg_edwards_unit* units, const kzg_derive_opts* opts,
                 uint8_t* out_commitments48, uint64_t* const out_stats[7], uint64_t* out_handle) {
    if (!ctx || !input_handles || !out_stats || !out_handle) return KZG_E_ARG;
    for (int k = 0; k < 7; k++)
        if (!out_stats[k]) return KZG_E_ARG;
    if (int rc = UnitCall::handles_ok(ctx, "edwards", n_input_handles)) return rc;
    if (n_units == 0 || n_units > KZG_EDWARDS_MAX_UNITS || !units)
        return fail(ctx, KZG_E_ARG, "edwards: n_units must be in [1, KZG_EDWARDS_MAX_UNITS]");
    if (!curve) return fail(ctx, KZG_E_ARG, "edwards: the curve must be given");
    static const uint8_t zero32[32] = {0};
    if (!fr_be32_canonical(curve->a_be32) || !fr_be32_canonical(curve->d_be32))
        return fail(ctx, KZG_E_ARG, "edwards: the coefficients A and D must be canonical scalars (< r)");
    if (!memcmp(curve->a_be32, zero32, 32) || !memcmp(curve->d_be32, zero32, 32))
        return fail(ctx, KZG_E_ARG, "edwards: the coefficients A and D must not be 0");
    if (!memcmp(curve->a_be32, curve->d_be32, 32)) return fail(ctx, KZG_E_ARG, "edwards: the coefficients A and D must differ");
    uint32_t n_out = 0;
    SeenRows S;
    for (uint32_t u = 0; u < n_units; u++) {
        const kzg_edwards_unit& U = units[u];
        if (U.mode != KZG_EDWARDS_ADD && U.mode != KZG_EDWARDS_CHAIN)
            return fail(ctx, KZG_E_ARG, "edwards: unknown mode (KZG_EDWARDS_ADD or KZG_EDWARDS_CHAIN)");
        if (U.flags & ~KZG_EDWARDS_CHECK) return fail(ctx, KZG_E_ARG, "edwards: flags must be 0 or KZG_EDWARDS_CHECK");
        const bool check = U.flags & KZG_EDWARDS_CHECK, chain = U.mode == KZG_EDWARDS_CHAIN;
        if (check && chain) return fail(ctx, KZG_E_ARG, "edwards: expect (KZG_EDWARDS_CHECK) belongs to ADD units, not to CHAIN");
        if (!U.cols || (U.cols & ~3u))
            return fail(ctx, KZG_E_ARG, "edwards: cols must name at least one column, and only columns of the unit's mode");
        const uint32_t n_in = chain ? 2u : 4u;
        for (uint32_t w = 0; w < 4; w++) {
            const bool takes = w < n_in, imm = U.in[w] == KZG_EDWARDS_IMM;
            if (takes != (U.in[w] != KZG_EDWARDS_ABSENT))
                return fail(ctx, KZG_E_ARG, "edwards: an operand the mode does not take, or a missing one (KZG_EDWARDS_ABSENT beside the mode's operands)");
            if (takes && imm) {
                if (!fr_be32_canonical(U.imm_be32[w])) return fail(ctx, KZG_E_ARG, "edwards: immediates must be canonical scalars (< r)");
            } else {
                if (memcmp(U.imm_be32[w], zero32, 32)) return fail(ctx, KZG_E_ARG, "edwards: the immediate must be 0 beside a row");
                if (takes) S.see(U.in[w]);
            }
        }
        if (chain != (U.op != KZG_EDWARDS_ABSENT))
            return fail(ctx, KZG_E_ARG, "edwards: op belongs to CHAIN units, and a CHAIN unit must have one (KZG_EDWARDS_ABSENT elsewhere)");
        if (chain) {
            if (U.op == KZG_EDWARDS_IMM) return fail(ctx, KZG_E_ARG, "edwards: op must be a row, not an immediate");
            S.see(U.op);
        }
        uint32_t ordered = 0;
        for (uint32_t k = 0; k < 2; k++) {
            const bool takes = check && (U.cols >> k & 1u);
            if (takes != (U.expect[k] != KZG_EDWARDS_ABSENT) || U.expect[k] == KZG_EDWARDS_IMM)
                return fail(ctx, KZG_E_ARG, "edwards: expect must hold one row per name of cols under KZG_EDWARDS_CHECK, KZG_EDWARDS_ABSENT elsewhere");
            if (takes) S.see(U.expect[k]);
            const uint32_t o = U.out_order[k];
            if (o == KZG_EDWARDS_ABSENT) continue;
            if (check || o > 1 || (ordered >> o & 1u) || (k == 1 && U.out_order[0] == KZG_EDWARDS_ABSENT))
                return fail(ctx, KZG_E_ARG, "edwards: out_order must list the names of cols once each (KZG_EDWARDS_ABSENT beyond, and in a check)");
            ordered |= 1u << o;
        }
        if (!check && ordered != U.cols)
            return fail(ctx, KZG_E_ARG, "edwards: out_order must list the names of cols once each (KZG_EDWARDS_ABSENT beyond, and in a check)");
        if (S.too_many())
            return fail(ctx, KZG_E_ARG, "edwards: a call reads at most KZG_MAX_BATCH_OPEN distinct input rows");
        n_out += check ? 0 : (uint32_t)__builtin_popcount(U.cols);
    }
    if (n_out > KZG_MAX_BATCH_OPEN)
        return fail(ctx, KZG_E_ARG, "edwards: n_out, the committed rows of all units, must be at most KZG_MAX_BATCH_OPEN");
    if (n_out && !out_commitments48) return KZG_E_ARG;
    UnitCall C(ctx, "edwards");
    if (int rc = C.open(expect_i, n_input_handles, input_handles, S.n != 0, S.max_row, ROW_WHY, n_out, opts)) return rc;
    uint64_t stats[5 * KZG_EDWARDS_MAX_UNITS];
    if (int rc = rows_edwards_dev(ctx, C.H, C.i, C.it, curve, n_units, units, n_out, C.T, C.dst(), C.c48, stats, C.blind)) return rc;
    // the device's runs: singular, mismatch or unknown, segments, first_singular, first of the second
    static const int run_of[7] = {0, 3, -1, -1, -1, -1, 2};
    bool chain[KZG_EDWARDS_MAX_UNITS];
    for (uint32_t u = 0; u < n_units; u++) chain[u] = units[u].mode == KZG_EDWARDS_CHAIN;
    stats_scatter(out_stats, run_of, 7, stats, n_units);
    stats_split(out_stats, 1, 2, 4, 0, stats, n_units, chain);
    stats_split(out_stats, 4, 3, 5, KZG_EDWARDS_NONE, stats, n_units, chain);
    C.finish(out_commitments48, out_handle);
    return KZG_OK;
}

// The terms of an expression as rows_expr_dev takes them: a kzg_quotient_terms checked (counts, lengths, canonical
// coefficients) and copied into the zeroed plan `pl`, its rotations as given into `rots` -- they are reduced by expr_reduce once
// T is known -- and the largest row it names into *max_row.  may_be_empty: n_terms = 0 is accepted and leaves pl empty
struct ExprRots {
    int32_t r[EXPR_MAX_TERMS][EXPR_MAX_FACTORS];
};
static int expr_decode(kzg_ctx* ctx, const char* what, const kzg_quotient_terms& g, bool may_be_empty, ExprPlan& pl, ExprRots& rots,
                       uint32_t* max_row) {
    auto bad = [&](const char* why) { return fail(ctx, KZG_E_ARG, std::string(what) + why); };
    if (g.n_terms > KZG_MAX_GATE_TERMS || (g.n_terms == 0 && !may_be_empty))
        return bad(may_be_empty ? ": n_terms must be in [0, KZG_MAX_GATE_TERMS]" : ": n_terms must be in [1, KZG_MAX_GATE_TERMS]");
    if (g.n_terms == 0) return KZG_OK;
    if (!g.coeffs_be32 || !g.term_lens) return bad(": coeffs_be32 and term_lens must not be null inside an expression");
    pl.n_terms = g.n_terms;
    pl.coeffs_be32 = g.coeffs_be32;
    for (uint32_t u = 0, at = 0; u < g.n_terms; u++) {
        if (!fr_be32_canonical(g.coeffs_be32 + 32 * (size_t)u)) return bad(": term coefficients must be canonical scalars (< r)");
        if (g.term_lens[u] > KZG_MAX_EXPR_FACTORS) return bad(": a term has more than KZG_MAX_EXPR_FACTORS factors");
        if (g.term_lens[u] && !g.term_rows) return bad(": term_rows must not be null inside an expression that has a factor");
        pl.term_len[u] = (uint8_t)g.term_lens[u];
        for (uint32_t f = 0; f < g.term_lens[u]; f++, at++) {
            *max_row = std::max(*max_row, g.term_rows[at]);
            pl.term_row[u][f] = (uint8_t)(g.term_rows[at] < KZG_MAX_BATCH_OPEN ? g.term_rows[at] : 0);
            if (g.term_rots) rots.r[u][f] = g.term_rots[at];
        }
    }
    return KZG_OK;
}
// any int32 rotation, reduced into [0, T)
static void expr_reduce(ExprPlan& pl, const ExprRots& rots, uint64_t T) {
    for (uint32_t u = 0; u < pl.n_terms; u++)
        for (uint32_t f = 0; f < pl.term_len[u]; f++)
            pl.term_rot[u][f] = (uint32_t)(((int64_t)rots.r[u][f] % (int64_t)T + (int64_t)T) % (int64_t)T);
}

// kzg_rows_commit_expr: the lookups of an open (one handle list), the reservation of a commit of n_out rows -- none when every
// expression is a check.  opts == NULL, or usable == 0: all T rows are evaluated.  Coefficients are checked here, on the host
int rows_expr(kzg_ctx* ctx, uint32_t expect_i, uint32_t n_input_handles, const uint64_t* input_handles, uint32_t n_exprs,
              const kzg_expr* exprs, const kzg_expr_opts* opts, uint8_t* out_commitments48, uint64_t* out_nonzero,
              uint64_t* out_first, uint64_t* out_handle) {
    if (!ctx || !input_handles || !out_nonzero || !out_first || !out_handle) return KZG_E_ARG;
    if (n_input_handles == 0 || n_input_handles > KZG_MAX_BATCH_OPEN)
        return fail(ctx, KZG_E_ARG, "expr: the number of handles must be in [1, KZG_MAX_BATCH_OPEN]");
    if (n_exprs == 0 || n_exprs > KZG_MAX_BATCH_OPEN || !exprs)
        return fail(ctx, KZG_E_ARG, "expr: n_exprs must be in [1, KZG_MAX_BATCH_OPEN]");
    ExprPlan plan[KZG_MAX_BATCH_OPEN];
    ExprRots rots[KZG_MAX_BATCH_OPEN];   // as given: reduced mod T once T is known
    uint8_t is_check[KZG_MAX_BATCH_OPEN];
    uint32_t n_out = 0, max_row = 0;
    memset(plan, 0, sizeof(plan));
    memset(rots, 0, sizeof(rots));
    for (uint32_t e = 0; e < n_exprs; e++) {
        if (exprs[e].flags & ~KZG_EXPR_CHECK) return fail(ctx, KZG_E_ARG, "expr: flags must be 0 or KZG_EXPR_CHECK");
        is_check[e] = exprs[e].flags == KZG_EXPR_CHECK;
        n_out += !is_check[e];
        if (int rc = expr_decode(ctx, "expr", exprs[e].terms, false, plan[e], rots[e], &max_row)) return rc;
    }
    if (n_out && !out_commitments48) return KZG_E_ARG;
    BuilderCall C(ctx, "expr");
    RowTab it;
    uint32_t ki = 0;
    if (int rc = C.begin("expr", expect_i, n_input_handles, input_handles, it, &ki)) return rc;
    if (max_row >= ki) return fail(ctx, KZG_E_ARG, "expr: a row must index the concatenated rows of the input sets");
    if (int rc = C.ready(n_out, 32, {opts ? opts->usable : 0, opts ? opts->tail_be32 : nullptr}, LAY_EVALUATED)) return rc;
    for (uint32_t e = 0; e < n_exprs; e++) expr_reduce(plan[e], rots[e], C.T);
    uint8_t c48[KZG_MAX_BATCH_OPEN * 48];
    uint64_t nonzero[KZG_MAX_BATCH_OPEN], first[KZG_MAX_BATCH_OPEN];
    if (int rc = rows_expr_dev(ctx, C.H, C.i, it, n_exprs, plan, is_check, n_out, C.T, C.dst(), c48, nonzero, first, C.blind))
        return rc;
    if (n_out) memcpy(out_commitments48, c48, 48 * (size_t)n_out);
    memcpy(out_nonzero, nonzero, 8 * (size_t)n_exprs);
    memcpy(out_first, first, 8 * (size_t)n_exprs);
    *out_handle = C.commit();
    return KZG_OK;
}

// kzg_rows_commit_recurrence: the lookups of an open (one handle list), the reservation of a commit of n_recs rows.  Each side
// of a recurrence is checked as rows_expr checks an expression, except that it may be empty (not both).  Coefficients and
// starts are checked here, on the host, before a lane is taken.  opts == NULL, or usable == 0: the plain layout
int rows_recurrence(kzg_ctx* ctx, uint32_t expect_i, uint32_t n_input_handles, const uint64_t* input_handles, uint32_t n_recs,
                    const kzg_recurrence* recs, const kzg_recurrence_opts* opts, uint8_t* out_commitments48,
                    uint8_t* out_closings32, uint64_t* out_handle) {
    if (!ctx || !input_handles || !out_commitments48 || !out_closings32 || !out_handle) return KZG_E_ARG;
    if (n_input_handles == 0 || n_input_handles > KZG_MAX_BATCH_OPEN)
        return fail(ctx, KZG_E_ARG, "recur: the number of handles must be in [1, KZG_MAX_BATCH_OPEN]");
    if (n_recs == 0 || n_recs > KZG_MAX_BATCH_OPEN || !recs)
        return fail(ctx, KZG_E_ARG, "recur: n_recs must be in [1, KZG_MAX_BATCH_OPEN]");
    std::vector<RecurSpec> spec(n_recs);
    std::vector<ExprRots> rots((size_t)n_recs * 2);   // mul, add of every recurrence, as given: reduced mod T once T is known
    uint32_t max_row = 0;
    for (uint32_t e = 0; e < n_recs; e++) {
        memset(&spec[e], 0, sizeof(RecurSpec));
        if (recs[e].mul.n_terms == 0 && recs[e].add.n_terms == 0)
            return fail(ctx, KZG_E_ARG, "recur: mul and add must not both be empty (v would be the constant start)");
        if (!recs[e].start_be32) return fail(ctx, KZG_E_ARG, "recur: start_be32 must not be null");
        if (!fr_be32_canonical(recs[e].start_be32)) return fail(ctx, KZG_E_ARG, "recur: start must be a canonical scalar (< r)");
        spec[e].start_be32 = recs[e].start_be32;
        if (int rc = expr_decode(ctx, "recur", recs[e].mul, true, spec[e].mul, rots[2 * e], &max_row)) return rc;
        if (int rc = expr_decode(ctx, "recur", recs[e].add, true, spec[e].add, rots[2 * e + 1], &max_row)) return rc;
    }
    BuilderCall C(ctx, "recur");
    RowTab it;
    uint32_t ki = 0;
    if (int rc = C.begin("recur", expect_i, n_input_handles, input_handles, it, &ki)) return rc;
    if (max_row >= ki) return fail(ctx, KZG_E_ARG, "recur: a row must index the concatenated rows of the input sets");
    // (the _zk layout over n_recs columns: blind_check's refusals, the tail column-major)
    if (int rc = C.ready(n_recs, 32, {opts ? opts->usable : 0, opts ? opts->tail_be32 : nullptr}, LAY_CLOSING)) return rc;
    for (uint32_t e = 0; e < n_recs; e++) {
        expr_reduce(spec[e].mul, rots[2 * e], C.T);
        expr_reduce(spec[e].add, rots[2 * e + 1], C.T);
    }
    uint8_t c48[KZG_MAX_BATCH_OPEN * 48], closing[KZG_MAX_BATCH_OPEN * 32];
    if (int rc = rows_recur_dev(ctx, C.H, C.i, it, n_recs, spec.data(), C.T, C.dst(), c48, closing, C.blind)) return rc;
    memcpy(out_commitments48, c48, 48 * (size_t)n_recs);
    memcpy(out_closings32, closing, 32 * (size_t)n_recs);
    *out_handle = C.commit();
    return KZG_OK;
}

// kzg_rows_commit_fetch: the lookups of an open (two handle lists, as rows_multiplicities), the reservation of a commit of
// n_out = n_reads (n_pay + index) rows.  What needs no set is refused before a lane is taken; w_tab is what the table sets hold.
// opts == NULL, or usable == 0: all T cells are read and all T table rows can answer
int rows_fetch(kzg_ctx* ctx, uint32_t expect_i, uint32_t n_input_handles, const uint64_t* input_handles, uint32_t n_table_handles,
               const uint64_t* table_handles, uint32_t n_reads, uint32_t n_keys, uint32_t flags, const kzg_derive_opts* opts,
               uint8_t* out_commitments48, uint64_t* out_missing, uint64_t* out_first_missing, uint64_t* out_handle) {
    if (!ctx || !input_handles || !table_handles || !out_commitments48 || !out_missing || !out_first_missing || !out_handle)
        return KZG_E_ARG;
    if (n_input_handles == 0 || n_input_handles > KZG_MAX_BATCH_OPEN || n_table_handles == 0 || n_table_handles > KZG_MAX_BATCH_OPEN)
        return fail(ctx, KZG_E_ARG, "fetch: the number of handles in each list must be in [1, KZG_MAX_BATCH_OPEN]");
    if (n_reads == 0) return fail(ctx, KZG_E_ARG, "fetch: n_reads must be at least 1");
    if (flags & ~KZG_FETCH_INDEX) return fail(ctx, KZG_E_ARG, "fetch: flags must be 0 or KZG_FETCH_INDEX");
    const bool index = flags == KZG_FETCH_INDEX;
    if (index && n_keys == 0)
        return fail(ctx, KZG_E_ARG, "fetch: KZG_FETCH_INDEX needs n_keys >= 1 (by row index the address column is the index)");
    const uint64_t n_in = (uint64_t)n_reads * (n_keys ? n_keys : 1);
    if (n_in > KZG_MAX_BATCH_OPEN)
        return fail(ctx, KZG_E_ARG, "fetch: n_reads * max(n_keys, 1) input rows must be at most KZG_MAX_BATCH_OPEN");
    BuilderCall C(ctx, "fetch");
    RowTab it, tt;
    uint32_t ki = 0, w_tab = 0;
    if (int rc = C.begin("fetch: inputs", expect_i, n_input_handles, input_handles, it, &ki)) return rc;
    if (int rc = C.lookup("fetch: table", expect_i, n_table_handles, table_handles, tt, &w_tab)) return rc;
    if (n_keys > w_tab) return fail(ctx, KZG_E_ARG, "fetch: n_keys must be at most the number of table rows");
    const uint32_t n_per = w_tab - n_keys + (index ? 1u : 0u);
    if (n_per == 0)
        return fail(ctx, KZG_E_ARG, "fetch: nothing to output: every table row is a key and KZG_FETCH_INDEX is not set");
    const uint64_t n_out = (uint64_t)n_reads * n_per;
    if (n_out > KZG_MAX_BATCH_OPEN)
        return fail(ctx, KZG_E_ARG, "fetch: n_reads * (payload rows + index) output rows must be at most KZG_MAX_BATCH_OPEN");
    if (ki != n_in) return fail(ctx, KZG_E_ARG, "fetch: the input sets must hold exactly n_reads * max(n_keys, 1) rows");
    // (2^27: a slot holds a u32 row index, 2 T slots a u32 offset)
    if (int rc = C.ready((uint32_t)n_out, 27, {opts ? opts->usable : 0, opts ? opts->tail_be32 : nullptr}, LAY_READ)) return rc;
    bool overrun = false;
    uint8_t c48[KZG_MAX_BATCH_OPEN * 48];
    uint64_t missing[KZG_MAX_BATCH_OPEN], first[KZG_MAX_BATCH_OPEN];
    if (int rc = rows_fetch_dev(ctx, C.H, C.i, it, tt, n_reads, n_keys, w_tab, index, C.T, C.dst(), c48, missing, first, &overrun,
                                C.blind))
        return rc;
    if (overrun)
        return fail(ctx, KZG_E_HIP, "fetch: a probe walk of the hash join reached its bound (the slot table held no empty "
                                    "slot): no set was created");
    memcpy(out_commitments48, c48, 48 * (size_t)n_out);
    memcpy(out_missing, missing, 8 * (size_t)n_reads);
    memcpy(out_first_missing, first, 8 * (size_t)n_reads);
    *out_handle = C.commit();
    return KZG_OK;
}

// The check of a _sel builder's selector arguments (SelCall, rows_impl.h): sel_index[l] is KZG_NO_SELECTOR or indexes the
// concatenated rows of the sel_handles sets, which must be of the call's worker and row length.  The distinct rows named go
// into sp (a row that serves several lookups is transformed once).
static int sel_plan(kzg_ctx* ctx, const char* what, uint32_t expect_i, const SelCall& sc, uint32_t n_lookups, uint32_t i, uint64_t T,
                    RowsRefs& refs, SelPlan& sp) {
    auto bad = [&](const char* why) { return fail(ctx, KZG_E_ARG, std::string(what) + why); };
    memset(&sp, 0, sizeof(sp));
    RowTab st;
    uint32_t ks = 0;
    if (sc.n_sel_handles) {
        uint32_t is = 0;
        uint64_t Ts = 0;
        if (int rc = rows_lookup(ctx, (std::string(what) + " (selectors)").c_str(), expect_i, sc.n_sel_handles, sc.sel_handles, refs,
                                 st, &ks, &is, &Ts))
            return rc;
        if (is != i || Ts != T) return bad(": all sets must belong to one worker and have one row length");
    }
    uint8_t slot_of[KZG_MAX_BATCH_OPEN];
    memset(slot_of, SEL_NONE, sizeof(slot_of));
    for (uint32_t l = 0; l < n_lookups; l++) {
        const uint32_t j = sc.sel_index[l];
        sp.of[l] = SEL_NONE;
        if (j == KZG_NO_SELECTOR) continue;
        if (j >= ks) return bad(": a sel_index entry must be KZG_NO_SELECTOR or index the concatenated rows of the selector sets");
        if (slot_of[j] == SEL_NONE) {
            slot_of[j] = (uint8_t)sp.n;
            sp.row[sp.n++] = st.r[j];
        }
        sp.of[l] = slot_of[j];
    }
    return KZG_OK;
}
// the layout of a _sel builder once T is known: usable == T with no tail is the plain layout (null), anything else the _zk
// call's, which blind_check then judges (so usable == T WITH a tail is its "usable must be in [1, T - 1]")
static const Blind* sel_layout(const Blind* zk, uint64_t T) { return zk->usable == T && !zk->tail_be32 ? nullptr : zk; }

// kzg_rows_commit_lookup_sum: the lookups of an open (three handle lists), the reservation of a commit.  zk: the blinding
// rows of kzg_rows_commit_lookup_sum_zk (null: the plain call).  sc: the selectors of kzg_rows_commit_lookup_sum_sel, one call
// for both layouts (sel_layout decides once T is known)
int rows_lookup_sum(kzg_ctx* ctx, uint32_t expect_i, uint32_t n_input_handles, const uint64_t* input_handles,
                    uint32_t n_table_handles, const uint64_t* table_handles, uint64_t mult_handle, uint32_t n_lookups,
                    uint32_t width, const uint8_t* theta_be32, const uint8_t* beta_be32, uint8_t* out_commitment48,
                    uint8_t* out_closing32, uint64_t* out_handle, const Blind* zk, const SelCall* sc) {
    if (!ctx || !input_handles || !table_handles || !theta_be32 || !beta_be32 || !out_commitment48 || !out_closing32 ||
        !out_handle)
        return KZG_E_ARG;
    if (sc && (!sc->sel_index || (sc->n_sel_handles && !sc->sel_handles))) return KZG_E_ARG;
    if (sc && sc->n_sel_handles > KZG_MAX_BATCH_OPEN)
        return fail(ctx, KZG_E_ARG, "lookup sum: at most KZG_MAX_BATCH_OPEN selector handles");
    if (n_input_handles == 0 || n_input_handles > KZG_MAX_BATCH_OPEN || n_table_handles == 0 || n_table_handles > KZG_MAX_BATCH_OPEN)
        return fail(ctx, KZG_E_ARG, "lookup sum: the number of handles in each list must be in [1, KZG_MAX_BATCH_OPEN]");
    if (n_lookups == 0 || width == 0 || (uint64_t)n_lookups * width > KZG_MAX_BATCH_OPEN)
        return fail(ctx, KZG_E_ARG, "lookup sum: n_lookups and width must be at least 1 and n_lookups * width at most "
                                    "KZG_MAX_BATCH_OPEN");
    if (!fr_be32_canonical(theta_be32) || !fr_be32_canonical(beta_be32))
        return fail(ctx, KZG_E_ARG, "lookup sum: theta and beta must be canonical scalars (< r)");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    RowsPending pend{ctx};
    RowsRefs irefs{ctx}, trefs{ctx}, mrefs{ctx}, srefs{ctx};
    LaneHold H(ctx);
    if (int rc = H.take()) return rc;   // (before the lookups: an SRS load cannot free the sets' buffers under this call)
    Lane& L = H.L();
    RowTab it, tt, mt;
    uint32_t ki = 0, kt = 0, km = 0, i = 0, i2 = 0, i3 = 0;
    uint64_t T = 0, T2 = 0, T3 = 0;
    if (int rc = rows_lookup(ctx, "lookup sum (inputs)", expect_i, n_input_handles, input_handles, irefs, it, &ki, &i, &T)) return rc;
    if (int rc = rows_lookup(ctx, "lookup sum (table)", expect_i, n_table_handles, table_handles, trefs, tt, &kt, &i2, &T2)) return rc;
    if (int rc = rows_lookup(ctx, "lookup sum (multiplicities)", expect_i, 1, &mult_handle, mrefs, mt, &km, &i3, &T3)) return rc;
    if (i2 != i || i3 != i || T2 != T || T3 != T)
        return fail(ctx, KZG_E_ARG, "lookup sum: all sets must belong to one worker and have one row length");
    if (ki != n_lookups * width || kt != width)
        return fail(ctx, KZG_E_ARG, "lookup sum: the input sets must hold exactly n_lookups * width rows and the table sets "
                                    "exactly width rows");
    if (km != 1) return fail(ctx, KZG_E_ARG, "lookup sum: the multiplicity set must hold exactly one row");
    int rc = check_worker(ctx, i, T);
    if (rc) return rc;
    if (ilog2_exact(T) < 0) return fail(ctx, KZG_E_ARG, "lookup sum: the row length must be a power of two");
    SelPlan sp;
    if (sc) {
        if (int rcs = sel_plan(ctx, "lookup sum", expect_i, *sc, n_lookups, i, T, srefs, sp)) return rcs;
        zk = sel_layout(zk, T);
    }
    if (zk)
        if (int rcz = blind_check(ctx, "lookup sum", T, *zk)) return rcz;
    if (int rc2 = rows_reserve(ctx, "lookup sum", pend, (size_t)T * 32)) return rc2;
    prof_begin(ctx, L);
    rc = clear_flags(ctx, L);
    if (rc) return rc;
    bool zero_den = false;
    uint8_t c48[48], closing[32];
    rc = rows_lookup_sum_dev(ctx, H, i, it, tt, mt.r[0], n_lookups, width, T, theta_be32, beta_be32, pend.buf.as<uint32_t>(), c48,
                             closing, &zero_den, zk, sc ? &sp : nullptr);
    if (rc) return rc;
    if (zero_den)
        return fail(ctx, KZG_E_ARG, zk ? "lookup sum: zero denominator (some beta + F_l or beta + Tb vanishes on a usable row): "
                                         "S is undefined, no set was created"
                                       : "lookup sum: zero denominator (some beta + F_l or beta + Tb vanishes on the domain): "
                                         "S is undefined, no set was created");
    memcpy(out_commitment48, c48, 48);
    memcpy(out_closing32, closing, 32);
    *out_handle = rows_insert(ctx, pend, i, 1, T);
    return KZG_OK;
}

// kzg_rows_commit_multiplicities: the lookups of an open (two handle lists), the reservation of a commit.  zk: the blinding
// rows of kzg_rows_commit_multiplicities_zk (null: the plain call).  sc: the selectors of kzg_rows_commit_multiplicities_sel
int rows_multiplicities(kzg_ctx* ctx, uint32_t expect_i, uint32_t n_input_handles, const uint64_t* input_handles,
                        uint32_t n_table_handles, const uint64_t* table_handles, uint32_t n_lookups, uint32_t width,
                        uint8_t* out_commitment48, uint64_t* out_missing, uint64_t* out_handle, const Blind* zk,
                        const SelCall* sc) {
    if (!ctx || !input_handles || !table_handles || !out_commitment48 || !out_missing || !out_handle) return KZG_E_ARG;
    if (sc && (!sc->sel_index || (sc->n_sel_handles && !sc->sel_handles))) return KZG_E_ARG;
    if (sc && sc->n_sel_handles > KZG_MAX_BATCH_OPEN)
        return fail(ctx, KZG_E_ARG, "multiplicities: at most KZG_MAX_BATCH_OPEN selector handles");
    if (n_input_handles == 0 || n_input_handles > KZG_MAX_BATCH_OPEN || n_table_handles == 0 || n_table_handles > KZG_MAX_BATCH_OPEN)
        return fail(ctx, KZG_E_ARG, "multiplicities: the number of handles in each list must be in [1, KZG_MAX_BATCH_OPEN]");
    if (n_lookups == 0 || width == 0 || (uint64_t)n_lookups * width > KZG_MAX_BATCH_OPEN)
        return fail(ctx, KZG_E_ARG, "multiplicities: n_lookups and width must be at least 1 and n_lookups * width at most "
                                    "KZG_MAX_BATCH_OPEN");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    RowsPending pend{ctx};
    RowsRefs irefs{ctx}, trefs{ctx}, srefs{ctx};
    LaneHold H(ctx);
    if (int rc = H.take()) return rc;   // (before the lookups: an SRS load cannot free the sets' buffers under this call)
    Lane& L = H.L();
    RowTab it, tt;
    uint32_t ki = 0, kt = 0, i = 0, i2 = 0;
    uint64_t T = 0, T2 = 0;
    if (int rc = rows_lookup(ctx, "multiplicities: inputs", expect_i, n_input_handles, input_handles, irefs, it, &ki, &i, &T)) return rc;
    if (int rc = rows_lookup(ctx, "multiplicities: table", expect_i, n_table_handles, table_handles, trefs, tt, &kt, &i2, &T2)) return rc;
    if (i2 != i || T2 != T)
        return fail(ctx, KZG_E_ARG, "multiplicities: all sets must belong to one worker and have one row length");
    if (ki != n_lookups * width || kt != width)
        return fail(ctx, KZG_E_ARG, "multiplicities: the input sets must hold exactly n_lookups * width rows and the table "
                                    "sets exactly width rows");
    int rc = check_worker(ctx, i, T);
    if (rc) return rc;
    if (ilog2_exact(T) < 0) return fail(ctx, KZG_E_ARG, "multiplicities: the row length must be a power of two");
    if (T > ((uint64_t)1 << 27))   // L T additions fit a u32 counter, 2 T slots a u32 index
        return fail(ctx, KZG_E_ARG, "multiplicities: the row length must be at most 2^27");
    SelPlan sp;
    if (sc) {
        if (int rcs = sel_plan(ctx, "multiplicities", expect_i, *sc, n_lookups, i, T, srefs, sp)) return rcs;
        zk = sel_layout(zk, T);
    }
    if (zk)
        if (int rcz = blind_check(ctx, "multiplicities", T, *zk)) return rcz;
    if (int rc2 = rows_reserve(ctx, "multiplicities", pend, (size_t)T * 32)) return rc2;
    prof_begin(ctx, L);
    rc = clear_flags(ctx, L);
    if (rc) return rc;
    bool overrun = false;
    uint8_t c48[48];
    uint64_t missing = 0;
    rc = rows_multiplicities_dev(ctx, H, i, it, tt, n_lookups, width, T, pend.buf.as<uint32_t>(), c48, &missing, &overrun, zk,
                                 sc ? &sp : nullptr);
    if (rc) return rc;
    if (overrun)
        return fail(ctx, KZG_E_HIP, "multiplicities: a probe walk of the hash join reached its bound (the slot table held no "
                                    "empty slot): no set was created");
    memcpy(out_commitment48, c48, 48);
    *out_missing = missing;
    *out_handle = rows_insert(ctx, pend, i, 1, T);
    return KZG_OK;
}

// The constraints of a quotient call as the caller gave them, checked and turned into the kernels' plan before any lane is
// taken (kzg_rows_commit_quotient*, and kzg_rows_quotient_part, which has no n_pieces: null).  `plain` only words one message.
struct QuotCall {
    QuotPlan qp;
    int32_t rots[QUOT_MAX_TERMS][QUOT_MAX_FACTORS];   // as given: reduced mod T once T is known
    int32_t link_rot;
    uint32_t max_row;   // the largest row index named, checked against the rows once they are known
    bool any_row;
};
static int quot_plan(kzg_ctx* ctx, const kzg_quotient_terms* gate, const kzg_quotient_perm* perm, const kzg_quotient_link* link,
                     const kzg_quotient_lookup* lookup, const kzg_quotient_active* active, uint32_t ext_log,
                     const uint32_t* n_pieces, uint32_t n_handles, bool plain, QuotCall& C,
                     const kzg_quotient_selectors* selectors = nullptr) {
    const uint32_t k = perm ? perm->k : 0;
    if (selectors && !selectors->selector_rows) return fail(ctx, KZG_E_ARG, "quotient: selectors->selector_rows must not be null");
    if (selectors && !lookup) return fail(ctx, KZG_E_ARG, "quotient: selectors need a lookup part (lookup != NULL)");
    if (gate->n_terms && (!gate->coeffs_be32 || !gate->term_lens || !gate->term_rows)) return KZG_E_ARG;
    if (lookup && (!lookup->input_rows || !lookup->table_rows || !lookup->theta_be32 || !lookup->beta_be32 || !lookup->alpha_be32))
        return KZG_E_ARG;
    if (k && (!perm->wire_rows || !perm->sigma_rows || !perm->shifts_be32 || !perm->beta_be32 || !perm->gamma_be32 ||
              !perm->alpha_be32))
        return KZG_E_ARG;
    if (n_handles == 0 || n_handles > KZG_MAX_BATCH_OPEN)
        return fail(ctx, KZG_E_ARG, "quotient: the number of handles must be in [1, KZG_MAX_BATCH_OPEN]");
    if (ext_log < 1 || ext_log > 3) return fail(ctx, KZG_E_ARG, "quotient: ext_log must be 1, 2 or 3");
    const uint32_t E = 1u << ext_log;
    if (n_pieces && (*n_pieces == 0 || *n_pieces > E)) return fail(ctx, KZG_E_ARG, "quotient: n_pieces must be in [1, 2^ext_log]");
    if (gate->n_terms > KZG_MAX_GATE_TERMS) return fail(ctx, KZG_E_ARG, "quotient: more than KZG_MAX_GATE_TERMS gate terms");
    if (k > E) return fail(ctx, KZG_E_ARG, "quotient: the permutation part has k + 1 factors: k must not exceed 2^ext_log");
    if (active && k > E - 1)
        return fail(ctx, KZG_E_ARG, "quotient: with an active column the permutation part has k + 2 factors: k must not exceed "
                                    "2^ext_log - 1");
    if (link && k == 0) return fail(ctx, KZG_E_ARG, "quotient: a link needs a permutation part (perm->k > 0)");
    if (gate->n_terms == 0 && k == 0 && !lookup)
        return fail(ctx, KZG_E_ARG, plain ? "quotient: no gate term and no permutation part"
                                          : "quotient: no gate term, no permutation part and no lookup part");
    if (lookup) {
        const uint32_t L = lookup->n_lookups, w = lookup->width;
        if (L == 0 || w == 0 || (uint64_t)L * w > KZG_MAX_BATCH_OPEN)
            return fail(ctx, KZG_E_ARG, "quotient: n_lookups and width must be at least 1 and n_lookups * width at most "
                                        "KZG_MAX_BATCH_OPEN");
        if (L > E - 1)
            return fail(ctx, KZG_E_ARG, "quotient: the lookup part has n_lookups + 2 factors: n_lookups must not exceed "
                                        "2^ext_log - 1");
        if (active && L > E - 2)
            return fail(ctx, KZG_E_ARG, "quotient: with an active column the lookup part has n_lookups + 3 factors: n_lookups "
                                        "must not exceed 2^ext_log - 2");
        if (!fr_be32_canonical(lookup->theta_be32) || !fr_be32_canonical(lookup->beta_be32) ||
            !fr_be32_canonical(lookup->alpha_be32))
            return fail(ctx, KZG_E_ARG, "quotient: the lookup part's theta, beta and alpha must be canonical scalars (< r)");
        if (k && memcmp(lookup->alpha_be32, perm->alpha_be32, 32) != 0)
            return fail(ctx, KZG_E_ARG, "quotient: the permutation part and the lookup part must name one alpha");
    }
    memset(&C, 0, sizeof(C));
    QuotPlan& qp = C.qp;
    qp.ext_log = ext_log;
    qp.n_terms = gate->n_terms;
    qp.k = k;
    qp.term_coeffs_be32 = gate->coeffs_be32;
    auto name_row = [&](uint32_t row) {
        C.any_row = true;
        if (row > C.max_row) C.max_row = row;
        return (uint8_t)(row < KZG_MAX_BATCH_OPEN ? row : 0);
    };
    for (uint32_t u = 0, at = 0; u < gate->n_terms; u++) {
        if (!fr_be32_canonical(gate->coeffs_be32 + 32 * (size_t)u))
            return fail(ctx, KZG_E_ARG, "quotient: term coefficients must be canonical scalars (< r)");
        if (gate->term_lens[u] > E + 1)
            return fail(ctx, KZG_E_ARG, "quotient: a gate term has more than 2^ext_log + 1 factors");
        qp.term_len[u] = (uint8_t)gate->term_lens[u];
        for (uint32_t f = 0; f < gate->term_lens[u]; f++, at++) {
            qp.term_row[u][f] = name_row(gate->term_rows[at]);
            if (gate->term_rots && gate->term_rots[at]) C.rots[u][f] = gate->term_rots[at], qp.ext = 1;
        }
    }
    if (k) {
        if (!fr_be32_canonical(perm->beta_be32) || !fr_be32_canonical(perm->gamma_be32) || !fr_be32_canonical(perm->alpha_be32))
            return fail(ctx, KZG_E_ARG, "quotient: beta, gamma and alpha must be canonical scalars (< r)");
        for (uint32_t j = 0; j < k; j++) {
            if (!fr_be32_canonical(perm->shifts_be32 + 32 * (size_t)j))
                return fail(ctx, KZG_E_ARG, "quotient: shifts must be canonical scalars (< r)");
            qp.wire[j] = name_row(perm->wire_rows[j]);
            qp.sigma[j] = name_row(perm->sigma_rows[j]);
        }
        qp.z_row = name_row(perm->z_row);
        qp.shifts_be32 = perm->shifts_be32;
        qp.beta_be32 = perm->beta_be32;
        qp.gamma_be32 = perm->gamma_be32;
        qp.alpha_be32 = perm->alpha_be32;
    }
    if (lookup) {
        qp.ext = 1;
        qp.n_lookups = lookup->n_lookups;
        qp.width = lookup->width;
        for (uint32_t j = 0; j < qp.n_lookups * qp.width; j++) qp.in_row[j] = name_row(lookup->input_rows[j]);
        for (uint32_t j = 0; j < qp.width; j++) qp.tab_row[j] = name_row(lookup->table_rows[j]);
        qp.mult_row = name_row(lookup->mult_row);
        qp.sum_row = name_row(lookup->sum_row);
        qp.theta_be32 = lookup->theta_be32;
        qp.lbeta_be32 = lookup->beta_be32;
        qp.alpha_be32 = lookup->alpha_be32;
    }
    if (active) {
        qp.ext = qp.active = 1;
        qp.active_row = name_row(active->active_row);
    }
    if (selectors) {   // every entry KZG_NO_SELECTOR: sel stays 0 and the call is the one without selectors
        for (uint32_t l = 0; l < qp.n_lookups; l++) {
            const uint32_t r = selectors->selector_rows[l];
            qp.sel_row[l] = 0xffu;
            if (r == KZG_NO_SELECTOR) continue;
            qp.sel_row[l] = name_row(r);
            qp.sel = 1;
        }
    }
    if (link) {
        qp.ext = qp.link = 1;
        qp.link_row = name_row(link->prev_row);
        C.link_rot = link->rot;
    }
    return KZG_OK;
}
// ... and against the rows once the lookup has found them: row indices, the worker, the row length, the rotations mod T
static int quot_plan_rows(kzg_ctx* ctx, QuotCall& C, uint32_t n, uint32_t i, uint64_t T) {
    if (C.any_row && C.max_row >= n) return fail(ctx, KZG_E_ARG, "quotient: a row index is not below the number of rows named");
    int rc = check_worker(ctx, i, T);
    if (rc) return rc;
    if (ilog2_exact(T) < 0) return fail(ctx, KZG_E_ARG, "quotient: the row length must be a power of two");
    auto reduce = [&](int32_t rot) { return (uint32_t)(((int64_t)rot % (int64_t)T + (int64_t)T) % (int64_t)T); };
    for (uint32_t u = 0; u < C.qp.n_terms; u++)   // any int32 rotation, reduced into [0, T)
        for (uint32_t f = 0; f < C.qp.term_len[u]; f++) C.qp.term_rot[u][f] = reduce(C.rots[u][f]);
    C.qp.link_rot = reduce(C.link_rot);
    return KZG_OK;
}

// kzg_rows_commit_quotient_ext (and, with no rotation and no lookup part, kzg_rows_commit_quotient: `plain`, which only words
// one message): the lookups of an open (one handle list), the reservation of a commit
// active: the caller's column A of kzg_rows_commit_quotient_zk, a factor of P1 and LK1 (null: neither has it)
// selectors: those of kzg_rows_commit_quotient_sel (null: none)
int rows_quotient(kzg_ctx* ctx, uint32_t expect_i, uint32_t n_handles, const uint64_t* handles, const kzg_quotient_terms* gate,
                  const kzg_quotient_perm* perm, const kzg_quotient_lookup* lookup, const kzg_quotient_selectors* selectors,
                  const kzg_quotient_active* active, uint32_t ext_log, uint32_t n_pieces, uint8_t* out_commitments48,
                  uint64_t* out_handle, bool plain) {
    if (!ctx || !handles || !gate || !out_commitments48 || !out_handle) return KZG_E_ARG;
    QuotCall C;
    if (int rc = quot_plan(ctx, gate, perm, nullptr, lookup, active, ext_log, &n_pieces, n_handles, plain, C, selectors)) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    RowsPending pend{ctx};
    RowsRefs refs{ctx};
    LaneHold H(ctx);
    if (int rc = H.take()) return rc;   // (before the lookups: an SRS load cannot free the sets' buffers under this call)
    Lane& L = H.L();
    RowTab rt;
    uint32_t n = 0, i = 0;
    uint64_t T = 0;
    if (int rc = rows_lookup(ctx, "quotient", expect_i, n_handles, handles, refs, rt, &n, &i, &T)) return rc;
    if (int rc = quot_plan_rows(ctx, C, n, i, T)) return rc;
    if (int rc2 = rows_reserve(ctx, "quotient", pend, (size_t)n_pieces * T * 32)) return rc2;
    prof_begin(ctx, L);
    int rc = clear_flags(ctx, L);
    if (rc) return rc;
    bool bad_shape = false;
    uint8_t c48[48 * 8];
    rc = rows_quotient_dev(ctx, H, i, rt, n, T, C.qp, n_pieces, pend.buf.as<uint32_t>(), c48, &bad_shape);
    if (rc) return rc;
    if (bad_shape)
        return fail(ctx, KZG_E_ARG, "quotient: t has a nonzero coefficient at or above n_pieces * T: the constraints do not hold "
                                    "on the domain, or n_pieces is too small; no set was created");
    memcpy(out_commitments48, c48, 48 * (size_t)n_pieces);
    *out_handle = rows_insert(ctx, pend, i, n_pieces, T);
    return KZG_OK;
}

// ---- the quotient in parts (kzg_rows_quotient_part / kzg_rows_quotient_finish).  The accumulator is an entry of the set table
// (RowSet::acc): handle, cap, stats, staleness, release and free list are the sets'; rows_lookup refuses it everywhere else.
// the accumulator `h` for a part or the finish (under sets_mu inside; lane held): one reference into refs
static int acc_lookup(kzg_ctx* ctx, const char* what, uint32_t expect_i, uint64_t h, RowsRefs& refs, kzg_ctx::RowSet** out) {
    auto bad = [&](const char* why) { return fail(ctx, KZG_E_ARG, std::string(what) + why); };
    std::lock_guard<std::mutex> lk(ctx->sets_mu);
    auto it = ctx->sets.find(h);
    if (it == ctx->sets.end() || it->second.released) return bad(": unknown, released or consumed accumulator handle");
    kzg_ctx::RowSet& st = it->second;
    if (!st.acc) return bad(": the handle names a row set, not a quotient accumulator");
    if (st.stale)
        return bad(": the accumulator is stale (the SRS was reloaded, or an add into it failed on the device): release it and "
                   "add its parts again");
    if (expect_i != UINT32_MAX && st.i != expect_i) return bad(": the accumulator belongs to another worker");
    st.refs++;
    refs.h[refs.n++] = h;
    *out = &st;   // (map nodes do not move; the reference keeps this one from being erased)
    return KZG_OK;
}
// selectors: those of kzg_rows_quotient_part_sel (null: kzg_rows_quotient_part)
int rows_quotient_part(kzg_ctx* ctx, uint32_t expect_i, uint32_t n_handles, const uint64_t* handles,
                       const kzg_quotient_terms* gate, const kzg_quotient_perm* perm, const kzg_quotient_link* link,
                       const kzg_quotient_lookup* lookup, const kzg_quotient_selectors* selectors,
                       const kzg_quotient_active* active, uint32_t ext_log, const uint8_t* scale_be32, uint64_t* inout_acc) {
    if (!ctx || !handles || !gate || !inout_acc) return KZG_E_ARG;
    if (scale_be32 && !fr_be32_canonical(scale_be32))
        return fail(ctx, KZG_E_ARG, "quotient part: scale must be a canonical scalar (< r)");
    QuotCall C;
    if (int rc = quot_plan(ctx, gate, perm, link, lookup, active, ext_log, nullptr, n_handles, false, C, selectors)) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    RowsPending pend{ctx};
    RowsRefs refs{ctx}, arefs{ctx};
    LaneHold H(ctx);
    if (int rc = H.take()) return rc;   // (before the lookups: an SRS load cannot free the buffers under this call)
    Lane& L = H.L();
    RowTab rt;
    uint32_t n = 0, i = 0;
    uint64_t T = 0;
    if (int rc = rows_lookup(ctx, "quotient part", expect_i, n_handles, handles, refs, rt, &n, &i, &T)) return rc;
    if (int rc = quot_plan_rows(ctx, C, n, i, T)) return rc;
    const bool first = *inout_acc == 0;
    const uint64_t h = *inout_acc;
    kzg_ctx::RowSet* acc = nullptr;
    if (first) {
        if (int rc = rows_reserve(ctx, "quotient part", pend, ((size_t)T << ext_log) * 32)) return rc;
    } else {
        if (int rc = acc_lookup(ctx, "quotient part", expect_i, h, arefs, &acc)) return rc;
        if (acc->i != i || acc->T != T || acc->acc_ext_log != ext_log)
            return fail(ctx, KZG_E_ARG, "quotient part: the part's worker, row length and ext_log must be the accumulator's");
    }
    prof_begin(ctx, L);
    int rc = clear_flags(ctx, L);
    if (rc) return rc;
    rc = rows_quotient_front_dev(ctx, H, rt, n, T, C.qp);
    if (rc) return rc;
    // the add: under the accumulator's mutex from its launch to the end of the call (a first part has no one to wait for).  A
    // later part looks again once it holds the mutex: a finish or a failed add may have come in between.  Any failure behind
    // the launch leaves contents nobody can vouch for: the accumulator goes stale (only KZG_E_HIP can happen: every scalar
    // was checked on the host)
    std::unique_lock<std::mutex> alk;
    if (!first) {
        alk = std::unique_lock<std::mutex>(*acc->acc_mu);
        std::lock_guard<std::mutex> lk(ctx->sets_mu);
        if (acc->released || acc->stale)
            return fail(ctx, KZG_E_ARG, "quotient part: the accumulator was consumed, released or made stale meanwhile");
    }
    rc = rows_quotient_add_dev(ctx, H, T, ext_log, scale_be32, first ? pend.buf.as<uint32_t>() : acc->buf.as<uint32_t>(), first);
    if (rc) {
        if (!first) {
            std::lock_guard<std::mutex> lk(ctx->sets_mu);
            acc->stale = true;
        }
        return rc;
    }
    if (first) {
        const uint64_t nh = ++g_row_set_handles;
        std::lock_guard<std::mutex> lk(ctx->sets_mu);
        kzg_ctx::RowSet& st = ctx->sets[nh];
        st.i = i;
        st.k = 0;
        st.T = T;
        st.acc = true;
        st.acc_ext_log = ext_log;
        st.acc_mu.reset(new std::mutex);
        st.buf = std::move(pend.buf);
        ctx->sets_pending--;
        pend.reserved = false;
        *inout_acc = nh;
    }
    return KZG_OK;
}
int rows_quotient_finish(kzg_ctx* ctx, uint32_t expect_i, uint64_t acc_handle, uint32_t n_pieces, uint8_t* out_commitments48,
                         uint64_t* out_handle) {
    if (!ctx || !out_commitments48 || !out_handle) return KZG_E_ARG;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    RowsPending pend{ctx};
    RowsRefs arefs{ctx};
    LaneHold H(ctx);
    if (int rc = H.take()) return rc;
    Lane& L = H.L();
    kzg_ctx::RowSet* acc = nullptr;
    if (int rc = acc_lookup(ctx, "quotient finish", expect_i, acc_handle, arefs, &acc)) return rc;
    const uint32_t i = acc->i, ext_log = acc->acc_ext_log;
    const uint64_t T = acc->T;
    if (n_pieces == 0 || n_pieces > (1u << ext_log))
        return fail(ctx, KZG_E_ARG, "quotient finish: n_pieces must be in [1, 2^ext_log]");
    int rc = check_worker(ctx, i, T);
    if (rc) return rc;
    std::unique_lock<std::mutex> alk(*acc->acc_mu);   // no part is between its add's launch and its end
    {
        std::lock_guard<std::mutex> lk(ctx->sets_mu);
        if (acc->released || acc->stale)
            return fail(ctx, KZG_E_ARG, "quotient finish: the accumulator was consumed, released or made stale meanwhile");
    }
    if (int rc2 = rows_reserve(ctx, "quotient finish", pend, (size_t)n_pieces * T * 32)) return rc2;
    prof_begin(ctx, L);
    rc = clear_flags(ctx, L);
    if (rc) return rc;
    bool bad_shape = false;
    uint8_t c48[48 * 8];
    rc = rows_quotient_finish_dev(ctx, H, i, T, (int)ext_log, acc->buf.as<uint32_t>(), n_pieces, pend.buf.as<uint32_t>(), c48,
                                  &bad_shape);
    if (rc) return rc;
    if (bad_shape)
        return fail(ctx, KZG_E_ARG, "quotient finish: t has a nonzero coefficient at or above n_pieces * T: the constraints do not "
                                    "hold on the domain, or n_pieces is too small; no set was created and the accumulator stays");
    memcpy(out_commitments48, c48, 48 * (size_t)n_pieces);
    *out_handle = rows_insert(ctx, pend, i, n_pieces, T);
    {   // consumed: the handle is unlinked now, the buffer goes to the free list when this call's reference drops
        std::lock_guard<std::mutex> lk(ctx->sets_mu);
        acc->released = true;
    }
    return KZG_OK;
}

int rows_release(kzg_ctx* ctx, uint32_t expect_i, uint64_t handle) {
    if (!ctx) return KZG_E_ARG;
    std::lock_guard<std::mutex> lk(ctx->sets_mu);
    auto it = ctx->sets.find(handle);
    if (it == ctx->sets.end() || it->second.released)
        return fail(ctx, KZG_E_ARG, "row-set release: unknown or already released handle");
    if (expect_i != UINT32_MAX && it->second.i != expect_i)
        return fail(ctx, KZG_E_ARG, "row-set release: the set belongs to another worker");
    it->second.released = true;
    if (it->second.refs == 0) rows_retire(ctx, it);   // else the last open that reads it retires it
    return KZG_OK;
}


// width in bytes of a typed column's cell (0: no such kind)
static uint32_t col_width(uint32_t kind) {
    switch (kind) {
        case KZG_COL_BE32: return 32;
        case KZG_COL_U8: return 1;
        case KZG_COL_U16: return 2;
        case KZG_COL_U32: case KZG_COL_I32: return 4;
        case KZG_COL_U64: case KZG_COL_I64: return 8;
    }
    return 0;
}
// kzg_rows_read: the lookup of an open; the row is read in place under the call's reference (a read changes nothing, so it
// runs beside opens of the same set), transformed forward into lane scratch when the domain values are asked for, narrowed
// into the lane's output buffer and copied out once the lane's record -- which carries the two overflow words -- is back
int rows_read(kzg_ctx* ctx, uint32_t expect_i, uint32_t n_handles, const uint64_t* handles, uint32_t row, uint64_t first,
              uint64_t count, uint32_t kind, int evaluation_form, void* out, uint64_t* out_overflow) {
    if (!ctx || !handles || !out_overflow || (count && !out)) return KZG_E_ARG;
    if (n_handles == 0 || n_handles > KZG_MAX_BATCH_OPEN)
        return fail(ctx, KZG_E_ARG, "row-set read: the number of handles must be in [1, KZG_MAX_BATCH_OPEN]");
    const uint32_t width = col_width(kind);
    if (!width) return fail(ctx, KZG_E_ARG, "row-set read: unknown kind");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    RowsRefs refs{ctx};
    LaneHold H(ctx);
    if (int rc = H.take()) return rc;
    Lane& L = H.L();
    RowTab rt;
    uint32_t k = 0, i = 0;
    uint64_t T = 0;
    if (int rc = rows_lookup(ctx, "row-set read", expect_i, n_handles, handles, refs, rt, &k, &i, &T)) return rc;
    if (row >= k) return fail(ctx, KZG_E_ARG, "row-set read: row outside the concatenated sets");
    if (first > T || count > T - first) return fail(ctx, KZG_E_ARG, "row-set read: first + count exceeds the row length");
    const int lg = ilog2_exact(T);
    if (evaluation_form && lg < 0)
        return fail(ctx, KZG_E_ARG, "row-set read: the values on the domain need a row length that is a power of two");
    out_overflow[0] = 0;
    out_overflow[1] = UINT64_MAX;
    if (count == 0) {
        H.clean = true;
        return KZG_OK;
    }
    prof_begin(ctx, L);
    int rc = clear_flags(ctx, L);
    if (rc) return rc;
    const uint32_t* src = rt.r[row];
    if (evaluation_form && lg > 0) {
        uint32_t* tw = nullptr;
        rc = ensure_twiddles(ctx, L, lg, 0, &tw, nullptr);
        if (rc) return rc;
        HIPCHK(ctx, L.coeffB.ensure(T * 32));
        HIPCHK(ctx, L.ntt_mid.ensure(T * 48));
        Span sp(ctx, L, KZG_T_NTT);
        launch_fr_ntt(L.stream, src, L.coeffB.as<uint32_t>(), lg, tw, nullptr, L.ntt_mid.as<uint32_t>());
        src = L.coeffB.as<uint32_t>();
    }
    const uint64_t bytes = count * width;
    HIPCHK(ctx, L.out_be.ensure(bytes));
    uint64_t* ovf = reinterpret_cast<uint64_t*>(L.tail + TB_EVAL);   // comes back with the lane's record
    {
        Span sp(ctx, L, KZG_T_DECODE);
        HIPCHK(ctx, hipMemsetAsync(ovf, 0, 16, L.stream));
        launch_fr_narrow(L.stream, src, first, count, kind, L.out_be.as<uint8_t>(), ovf);
    }
    L.expect_short = true;   // one transform and one pass over a row, no MSM: finish() may poll for the record
    rc = finish(ctx, L);
    if (rc) return rc;
    HIPCHK(ctx, hipMemcpy(out, L.out_be.p, bytes, hipMemcpyDeviceToHost));
    uint64_t rec[2];
    memcpy(rec, L.pin + TB_EVAL, 16);
    out_overflow[0] = rec[0];
    out_overflow[1] = rec[1] ? UINT64_MAX - rec[1] : UINT64_MAX;
    H.clean = true;
    return KZG_OK;
}

}  // namespace kzg_impl

extern "C" {

// k rows of worker i committed and kept on the device as coefficients (pipeline.hip: rows_commit_dev)
int kzg_rows_commit(kzg_ctx* ctx, uint32_t i, uint32_t k, const uint8_t* rows_be32, uint64_t T, int evaluation_form,
                    uint8_t* out_commitments48, uint64_t* out_handle) {
    if (!ctx || !rows_be32 || !out_commitments48 || !out_handle) return KZG_E_ARG;
    if (k == 0 || k > KZG_MAX_BATCH_OPEN) return fail(ctx, KZG_E_ARG, "row-set commit: k must be in [1, KZG_MAX_BATCH_OPEN]");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    RowsPending pend{ctx};
    LaneHold H(ctx);
    if (int rc = H.take()) return rc;
    Lane& L = H.L();
    int rc = check_worker(ctx, i, T);
    if (rc) return rc;
    if (evaluation_form && T > 1 && ilog2_exact(T) < 0)
        return fail(ctx, KZG_E_ARG, "evaluation-form row length must be a power of two");
    const size_t bytes = (size_t)k * T * 32;
    if (int rc2 = rows_reserve(ctx, "row-set commit", pend, bytes)) return rc2;
    prof_begin(ctx, L);
    rc = clear_flags(ctx, L);
    if (rc) return rc;
    // evaluation-form rows are uploaded to the lane and transformed into the set's buffer; coefficient rows land there directly
    uint32_t* dst = pend.buf.as<uint32_t>();
    uint32_t* up = dst;
    if (evaluation_form && T > 1) {
        HIPCHK(ctx, L.coeffA.ensure(bytes));
        up = L.coeffA.as<uint32_t>();
    }
    rc = upload_fr(ctx, L, rows_be32, (uint64_t)k * T, up, 1);
    if (rc) return rc;
    rc = rows_commit_dev(ctx, H, i, up, k, T, evaluation_form, dst, out_commitments48);
    if (rc) return rc;
    const uint64_t h = rows_insert(ctx, pend, i, k, T);
    *out_handle = h;
    return KZG_OK;
}
// kzg_rows_commit with the rows as typed columns: everything but the upload and decode in front of rows_commit_dev is that
// call's.  The integer columns are packed into the lane's input buffer (each on a 16-byte boundary, one copy per column) and
// decoded by one launch; be32 columns go through the decoder of upload_fr, whose flag a cell >= r raises
int kzg_rows_commit_typed(kzg_ctx* ctx, uint32_t i, uint32_t k, const kzg_col* cols, uint64_t T, int evaluation_form,
                          uint8_t* out_commitments48, uint64_t* out_handle) {
    if (!ctx || !cols || !out_commitments48 || !out_handle) return KZG_E_ARG;
    if (k == 0 || k > KZG_MAX_BATCH_OPEN)
        return fail(ctx, KZG_E_ARG, "typed row-set commit: k must be in [1, KZG_MAX_BATCH_OPEN]");
    static_assert(KZG_MAX_BATCH_OPEN <= FR_TYPED_MAX_COLS, "one table holds every column of a call");
    TypedTab tab;
    memset(&tab, 0, sizeof(tab));
    uint64_t off[KZG_MAX_BATCH_OPEN], packed = 0;
    uint32_t n_typed = 0;
    for (uint32_t c = 0; c < k; c++) {
        const kzg_col& col = cols[c];
        const uint32_t width = col_width(col.kind);
        if (!width) return fail(ctx, KZG_E_ARG, "typed row-set commit: unknown column kind");
        if (col.count > T) return fail(ctx, KZG_E_ARG, "typed row-set commit: a column holds more than T cells");
        if (col.count && !col.data) return fail(ctx, KZG_E_ARG, "typed row-set commit: a column with cells has no data");
        if (col.fill_be32 && !fr_be32_canonical(col.fill_be32))
            return fail(ctx, KZG_E_ARG, "typed row-set commit: a fill must be a canonical scalar (< r)");
        off[c] = packed;
        packed += (col.count * width + 15) & ~(uint64_t)15;
        if (col.kind == KZG_COL_BE32 && col.count == T) continue;   // all cells through the be32 decoder: no fill to write
        TypedCol& e = tab.c[n_typed++];
        e.off = off[c];
        e.count = col.count;
        e.skip = col.kind == KZG_COL_BE32 ? col.count : 0;           // (a short be32 column: the launch writes its fill only)
        e.kind = col.kind;
        e.row = c;
        for (int w = 0; col.fill_be32 && w < 8; w++) {
            uint32_t be;
            memcpy(&be, col.fill_be32 + 4 * (7 - w), 4);
            e.fill[w] = __builtin_bswap32(be);
        }
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    RowsPending pend{ctx};
    LaneHold H(ctx);
    if (int rc = H.take()) return rc;
    Lane& L = H.L();
    int rc = check_worker(ctx, i, T);
    if (rc) return rc;
    if (evaluation_form && T > 1 && ilog2_exact(T) < 0)
        return fail(ctx, KZG_E_ARG, "evaluation-form row length must be a power of two");
    const size_t bytes = (size_t)k * T * 32;
    if (int rc2 = rows_reserve(ctx, "typed row-set commit", pend, bytes)) return rc2;
    prof_begin(ctx, L);
    rc = clear_flags(ctx, L);
    if (rc) return rc;
    uint32_t* dst = pend.buf.as<uint32_t>();
    uint32_t* up = dst;
    if (evaluation_form && T > 1) {
        HIPCHK(ctx, L.coeffA.ensure(bytes));
        up = L.coeffA.as<uint32_t>();
    }
    {
        Span sp(ctx, L, KZG_T_DECODE);
        HIPCHK(ctx, L.in_be.ensure(packed + 16));
        uint8_t* in = L.in_be.as<uint8_t>();
        for (uint32_t c = 0; c < k; c++)
            if (cols[c].count)
                HIPCHK(ctx, hipMemcpyAsync(in + off[c], cols[c].data, cols[c].count * col_width(cols[c].kind),
                                           hipMemcpyHostToDevice, L.stream));
        launch_fr_from_typed(L.stream, in, tab, n_typed, up, T);
        for (uint32_t c = 0; c < k; c++)   // (the launch above wrote a be32 column's cells at or behind `count` only)
            if (cols[c].kind == KZG_COL_BE32)
                launch_fr_from_be(L.stream, in + off[c], up + (uint64_t)c * T * 8, cols[c].count, 1, L.flags());
    }
    rc = rows_commit_dev(ctx, H, i, up, k, T, evaluation_form, dst, out_commitments48);
    if (rc == KZG_E_SCALAR) return fail(ctx, KZG_E_ARG, "typed row-set commit: a be32 cell is not a canonical scalar (< r)");
    if (rc) return rc;
    *out_handle = rows_insert(ctx, pend, i, k, T);
    return KZG_OK;
}
int kzg_rows_read(kzg_ctx* ctx, uint32_t n_handles, const uint64_t* handles, uint32_t row, uint64_t first, uint64_t count,
                  uint32_t kind, int evaluation_form, void* out, uint64_t out_overflow[2]) {
    return rows_read(ctx, UINT32_MAX, n_handles, handles, row, first, count, kind, evaluation_form, out, out_overflow);
}
// The exports below are the entries of rows_impl.h for any one worker (UINT32_MAX): what a variant adds goes in as a Blind / SelCall
// on the stack, what it lacks as null
int kzg_rows_open(kzg_ctx* ctx, uint32_t n_handles, const uint64_t* handles, uint32_t m, const uint8_t* points_be32,
                  const uint32_t* masks, const uint8_t* gammas_be32, uint8_t* out_evals32, uint8_t* out_proofs48) {
    return rows_open(ctx, UINT32_MAX, n_handles, handles, m, points_be32, masks, gammas_be32, out_evals32, out_proofs48);
}
int kzg_rows_eval(kzg_ctx* ctx, uint32_t n_handles, const uint64_t* handles, uint32_t m, const uint8_t* points_be32,
                  const uint32_t* masks, uint8_t* out_evals32) {
    return rows_eval(ctx, UINT32_MAX, n_handles, handles, m, points_be32, masks, out_evals32);
}
int kzg_rows_open_lincomb(kzg_ctx* ctx, uint32_t n_handles, const uint64_t* handles, uint32_t k, uint32_t m,
                          const uint8_t* points_be32, const uint8_t* coeffs_be32, uint8_t* out_values32, uint8_t* out_proofs48) {
    return rows_lincomb(ctx, UINT32_MAX, n_handles, handles, k, m, points_be32, coeffs_be32, out_values32, out_proofs48);
}
int kzg_rows_commit_shplonk(kzg_ctx* ctx, uint32_t n_handles, const uint64_t* handles, uint32_t k, uint32_t m,
                            const uint8_t* points_be32, const uint32_t* masks, const uint8_t* coeffs_be32,
                            uint8_t out_commitment48[48], uint64_t* out_handle) {
    return rows_shplonk(ctx, UINT32_MAX, n_handles, handles, k, m, points_be32, masks, coeffs_be32, out_commitment48, out_handle);
}
int kzg_rows_commit_grand_product(kzg_ctx* ctx, uint32_t n_wire_handles, const uint64_t* wire_handles, uint32_t n_sigma_handles,
                                  const uint64_t* sigma_handles, uint32_t k, const uint8_t* shifts_be32,
                                  const uint8_t beta_be32[32], const uint8_t gamma_be32[32], uint8_t out_commitment48[48],
                                  uint8_t out_closing32[32], uint64_t* out_handle) {
    return rows_grand_product(ctx, UINT32_MAX, n_wire_handles, wire_handles, n_sigma_handles, sigma_handles, k, shifts_be32,
                              beta_be32, gamma_be32, out_commitment48, out_closing32, out_handle, nullptr, nullptr);
}
int kzg_rows_commit_grand_product_zk(kzg_ctx* ctx, uint32_t n_wire_handles, const uint64_t* wire_handles,
                                     uint32_t n_sigma_handles, const uint64_t* sigma_handles, uint32_t k,
                                     const uint8_t* shifts_be32, const uint8_t beta_be32[32], const uint8_t gamma_be32[32],
                                     uint64_t usable, const uint8_t* tail_be32, uint8_t out_commitment48[48],
                                     uint8_t out_closing32[32], uint64_t* out_handle) {
    const Blind zk = {usable, tail_be32};
    return rows_grand_product(ctx, UINT32_MAX, n_wire_handles, wire_handles, n_sigma_handles, sigma_handles, k, shifts_be32,
                              beta_be32, gamma_be32, out_commitment48, out_closing32, out_handle, &zk, nullptr);
}
// the _zk call whose z starts at `start` instead of 1 (a null start is refused here: to the entry it means "not a chain")
int kzg_rows_commit_grand_product_chain(kzg_ctx* ctx, uint32_t n_wire_handles, const uint64_t* wire_handles,
                                        uint32_t n_sigma_handles, const uint64_t* sigma_handles, uint32_t k,
                                        const uint8_t* shifts_be32, const uint8_t beta_be32[32], const uint8_t gamma_be32[32],
                                        uint64_t usable, const uint8_t* tail_be32, const uint8_t start_be32[32],
                                        uint8_t out_commitment48[48], uint8_t out_closing32[32], uint64_t* out_handle) {
    if (!start_be32) return KZG_E_ARG;
    const Blind zk = {usable, tail_be32};
    return rows_grand_product(ctx, UINT32_MAX, n_wire_handles, wire_handles, n_sigma_handles, sigma_handles, k, shifts_be32,
                              beta_be32, gamma_be32, out_commitment48, out_closing32, out_handle, &zk, start_be32);
}
int kzg_rows_commit_shuffle(kzg_ctx* ctx, uint32_t n_input_handles, const uint64_t* input_handles, uint32_t n_shuffle_handles,
                            const uint64_t* shuffle_handles, uint32_t n_groups, uint32_t width, const uint8_t theta_be32[32],
                            const uint8_t gamma_be32[32], const kzg_shuffle_opts* opts, uint8_t out_commitment48[48],
                            uint8_t out_closing32[32], uint64_t* out_handle) {
    return rows_shuffle(ctx, UINT32_MAX, n_input_handles, input_handles, n_shuffle_handles, shuffle_handles, n_groups, width,
                        theta_be32, gamma_be32, opts, out_commitment48, out_closing32, out_handle);
}
int kzg_rows_commit_sorted(kzg_ctx* ctx, uint32_t n_input_handles, const uint64_t* input_handles, uint32_t width, uint32_t n_keys,
                           const kzg_sorted_opts* opts, uint8_t* out_commitments48, uint64_t* out_handle) {
    return rows_sorted(ctx, UINT32_MAX, n_input_handles, input_handles, width, n_keys, opts, out_commitments48, out_handle);
}
int kzg_rows_commit_sigma(kzg_ctx* ctx, uint32_t n_label_handles, const uint64_t* label_handles, uint32_t k,
                          const uint8_t* shifts_be32, const kzg_sigma_opts* opts, uint8_t* out_commitments48, uint64_t out_stats[2],
                          uint64_t* out_handle) {
    return rows_sigma(ctx, UINT32_MAX, n_label_handles, label_handles, k, shifts_be32, opts, out_commitments48, out_stats,
                      out_handle);
}
int kzg_rows_check_copies(kzg_ctx* ctx, uint32_t n_wire_handles, const uint64_t* wire_handles, uint32_t n_label_handles,
                          const uint64_t* label_handles, uint32_t k, const kzg_sigma_opts* opts, uint64_t out[2]) {
    return rows_check_copies(ctx, UINT32_MAX, n_wire_handles, wire_handles, n_label_handles, label_handles, k, opts, out);
}
int kzg_rows_commit_derived(kzg_ctx* ctx, uint32_t n_input_handles, const uint64_t* input_handles, uint32_t n_ops,
                            const kzg_derive_op* ops, const kzg_derive_opts* opts, uint8_t* out_commitments48,
                            uint64_t* out_counts, uint64_t* out_handle) {
    return rows_derived(ctx, UINT32_MAX, n_input_handles, input_handles, n_ops, ops, opts, out_commitments48, out_counts,
                        out_handle);
}
int kzg_rows_commit_int(kzg_ctx* ctx, uint32_t n_input_handles, const uint64_t* input_handles, uint32_t n_ops,
                        const kzg_int_op* ops, const kzg_derive_opts* opts, uint8_t* out_commitments48, uint64_t* out_counts,
                        uint64_t* out_first, uint64_t* out_handle) {
    return rows_int(ctx, UINT32_MAX, n_input_handles, input_handles, n_ops, ops, opts, out_commitments48, out_counts, out_first,
                    out_handle);
}
int kzg_rows_commit_alu(kzg_ctx* ctx, uint32_t n_input_handles, const uint64_t* input_handles, uint32_t n_entries,
                        const kzg_alu_entry* program, uint32_t n_units, const kzg_alu_unit* units, const kzg_derive_opts* opts,
                        uint8_t* out_commitments48, uint64_t* out_counts, uint64_t* out_first, uint64_t* out_unknown,
                        uint64_t* out_first_unknown, uint64_t* out_handle) {
    return rows_alu(ctx, UINT32_MAX, n_input_handles, input_handles, n_entries, program, n_units, units, opts,
                    out_commitments48, out_counts, out_first, out_unknown, out_first_unknown, out_handle);
}
int kzg_rows_commit_wide(kzg_ctx* ctx, uint32_t n_input_handles, const uint64_t* input_handles, uint32_t n_ops,
                         const kzg_wide_op* ops, const kzg_derive_opts* opts, uint8_t* out_commitments48, uint64_t* out_counts,
                         uint64_t* out_first, uint64_t* out_qover, uint64_t* out_first_qover, uint64_t* out_handle) {
    return rows_wide(ctx, UINT32_MAX, n_input_handles, input_handles, n_ops, ops, opts, out_commitments48, out_counts, out_first,
                     out_qover, out_first_qover, out_handle);
}
int kzg_rows_commit_poseidon_chain(kzg_ctx* ctx, uint32_t n_input_handles, const uint64_t* input_handles,
                                   const kzg_poseidon_params* params, uint32_t n_units, const kzg_poseidon_chain_unit* units,
                                   const kzg_derive_opts* opts, uint8_t* out_commitments48, uint64_t* out_blocks,
                                   uint64_t* out_segments, uint64_t* out_bad_pos, uint64_t* out_first_bad_pos,
                                   uint64_t* out_mismatch, uint64_t* out_first_mismatch, uint64_t* out_handle) {
    uint64_t* const st[6] = {out_blocks, out_segments, out_bad_pos, out_first_bad_pos, out_mismatch, out_first_mismatch};
    return rows_poseidon_chain(ctx, UINT32_MAX, n_input_handles, input_handles, params, n_units, units, opts, out_commitments48, st,
                               out_handle);
}
int kzg_rows_commit_poseidon(kzg_ctx* ctx, uint32_t n_input_handles, const uint64_t* input_handles,
                             const kzg_poseidon_params* params, uint32_t n_units, const kzg_poseidon_unit* units,
                             const kzg_derive_opts* opts, uint8_t* out_commitments48, uint64_t* out_perms, uint64_t* out_mismatch,
                             uint64_t* out_first_mismatch, uint64_t* out_handle) {
    return rows_poseidon(ctx, UINT32_MAX, n_input_handles, input_handles, params, n_units, units, opts, out_commitments48,
                         out_perms, out_mismatch, out_first_mismatch, out_handle);
}
int kzg_rows_commit_poseidon2(kzg_ctx* ctx, uint32_t n_input_handles, const uint64_t* input_handles,
                              const kzg_poseidon2_params* params, uint32_t n_units, const kzg_poseidon_unit* units,
                              const kzg_derive_opts* opts, uint8_t* out_commitments48, uint64_t* out_perms,
                              uint64_t* out_mismatch, uint64_t* out_first_mismatch, uint64_t* out_handle) {
    return rows_poseidon2(ctx, UINT32_MAX, n_input_handles, input_handles, params, n_units, units, opts, out_commitments48,
                          out_perms, out_mismatch, out_first_mismatch, out_handle);
}
int kzg_rows_commit_sha256(kzg_ctx* ctx, uint32_t n_input_handles, const uint64_t* input_handles, uint32_t n_units,
                           const kzg_sha256_unit* units, const kzg_derive_opts* opts, uint8_t* out_commitments48,
                           uint64_t* out_blocks, uint64_t* out_messages, uint64_t* out_counts, uint64_t* out_first,
                           uint64_t* out_mismatch, uint64_t* out_first_mismatch, uint64_t* out_handle) {
    return rows_sha256(ctx, UINT32_MAX, n_input_handles, input_handles, n_units, units, opts, out_commitments48, out_blocks,
                       out_messages, out_counts, out_first, out_mismatch, out_first_mismatch, out_handle);
}
int kzg_rows_commit_keccak(kzg_ctx* ctx, uint32_t n_input_handles, const uint64_t* input_handles, uint32_t n_units,
                           const kzg_keccak_unit* units, const kzg_derive_opts* opts, uint8_t* out_commitments48,
                           uint64_t* out_perms, uint64_t* out_messages, uint64_t* out_counts, uint64_t* out_first,
                           uint64_t* out_mismatch, uint64_t* out_first_mismatch, uint64_t* out_handle) {
    return rows_keccak(ctx, UINT32_MAX, n_input_handles, input_handles, n_units, units, opts, out_commitments48, out_perms,
                       out_messages, out_counts, out_first, out_mismatch, out_first_mismatch, out_handle);
}
int kzg_rows_commit_ec(kzg_ctx* ctx, uint32_t n_input_handles, const uint64_t* input_handles, const kzg_ec_curve* curve,
                       uint32_t n_units, const kzg_ec_unit* units, const kzg_derive_opts* opts, uint8_t* out_commitments48,
                       uint64_t* out_counts, uint64_t* out_first, uint64_t* out_singular, uint64_t* out_first_singular,
                       uint64_t* out_mismatch, uint64_t* out_first_mismatch, uint64_t* out_unknown, uint64_t* out_first_unknown,
                       uint64_t* out_segments, uint64_t* out_handle) {
    uint64_t* const st[9] = {out_counts,         out_first,   out_singular,      out_first_singular, out_mismatch,
                             out_first_mismatch, out_unknown, out_first_unknown, out_segments};
    return rows_ec(ctx, UINT32_MAX, n_input_handles, input_handles, curve, n_units, units, opts, out_commitments48, st, out_handle);
}
int kzg_rows_commit_edwards(kzg_ctx* ctx, uint32_t n_input_handles, const uint64_t* input_handles, const kzg_edwards_curve* curve,
                            uint32_t n_units, const kzg_edwards_unit* units, const kzg_derive_opts* opts,
                            uint8_t* out_commitments48, uint64_t* out_singular, uint64_t* out_first_singular,
                            uint64_t* out_mismatch, uint64_t* out_first_mismatch, uint64_t* out_unknown,
                            uint64_t* out_first_unknown, uint64_t* out_segments, uint64_t* out_handle) {
    uint64_t* const st[7] = {out_singular, out_first_singular, out_mismatch, out_first_mismatch,
                             out_unknown,  out_first_unknown,  out_segments};
    return rows_edwards(ctx, UINT32_MAX, n_input_handles, input_handles, curve, n_units, units, opts, out_commitments48, st,
                        out_handle);
}
int kzg_rows_commit_expr(kzg_ctx* ctx, uint32_t n_input_handles, const uint64_t* input_handles, uint32_t n_exprs,
                         const kzg_expr* exprs, const kzg_expr_opts* opts, uint8_t* out_commitments48, uint64_t* out_nonzero,
                         uint64_t* out_first, uint64_t* out_handle) {
    return rows_expr(ctx, UINT32_MAX, n_input_handles, input_handles, n_exprs, exprs, opts, out_commitments48, out_nonzero,
                     out_first, out_handle);
}
int kzg_rows_commit_recurrence(kzg_ctx* ctx, uint32_t n_input_handles, const uint64_t* input_handles, uint32_t n_recs,
                               const kzg_recurrence* recs, const kzg_recurrence_opts* opts, uint8_t* out_commitments48,
                               uint8_t* out_closings32, uint64_t* out_handle) {
    return rows_recurrence(ctx, UINT32_MAX, n_input_handles, input_handles, n_recs, recs, opts, out_commitments48,
                           out_closings32, out_handle);
}
int kzg_rows_commit_fetch(kzg_ctx* ctx, uint32_t n_input_handles, const uint64_t* input_handles, uint32_t n_table_handles,
                          const uint64_t* table_handles, uint32_t n_reads, uint32_t n_keys, uint32_t flags,
                          const kzg_derive_opts* opts, uint8_t* out_commitments48, uint64_t* out_missing,
                          uint64_t* out_first_missing, uint64_t* out_handle) {
    return rows_fetch(ctx, UINT32_MAX, n_input_handles, input_handles, n_table_handles, table_handles, n_reads, n_keys, flags, opts,
                      out_commitments48, out_missing, out_first_missing, out_handle);
}
int kzg_rows_commit_lookup_sum(kzg_ctx* ctx, uint32_t n_input_handles, const uint64_t* input_handles, uint32_t n_table_handles,
                               const uint64_t* table_handles, uint64_t mult_handle, uint32_t n_lookups, uint32_t width,
                               const uint8_t theta_be32[32], const uint8_t beta_be32[32], uint8_t out_commitment48[48],
                               uint8_t out_closing32[32], uint64_t* out_handle) {
    return rows_lookup_sum(ctx, UINT32_MAX, n_input_handles, input_handles, n_table_handles, table_handles, mult_handle, n_lookups,
                           width, theta_be32, beta_be32, out_commitment48, out_closing32, out_handle, nullptr, nullptr);
}
int kzg_rows_commit_lookup_sum_zk(kzg_ctx* ctx, uint32_t n_input_handles, const uint64_t* input_handles, uint32_t n_table_handles,
                                  const uint64_t* table_handles, uint64_t mult_handle, uint32_t n_lookups, uint32_t width,
                                  const uint8_t theta_be32[32], const uint8_t beta_be32[32], uint64_t usable,
                                  const uint8_t* tail_be32, uint8_t out_commitment48[48], uint8_t out_closing32[32],
                                  uint64_t* out_handle) {
    const Blind zk = {usable, tail_be32};
    return rows_lookup_sum(ctx, UINT32_MAX, n_input_handles, input_handles, n_table_handles, table_handles, mult_handle, n_lookups,
                           width, theta_be32, beta_be32, out_commitment48, out_closing32, out_handle, &zk, nullptr);
}
int kzg_rows_commit_lookup_sum_sel(kzg_ctx* ctx, uint32_t n_input_handles, const uint64_t* input_handles, uint32_t n_table_handles,
                                   const uint64_t* table_handles, uint64_t mult_handle, uint32_t n_sel_handles,
                                   const uint64_t* sel_handles, const uint32_t* sel_index, uint32_t n_lookups, uint32_t width,
                                   const uint8_t theta_be32[32], const uint8_t beta_be32[32], uint64_t usable,
                                   const uint8_t* tail_be32, uint8_t out_commitment48[48], uint8_t out_closing32[32],
                                   uint64_t* out_handle) {
    const Blind zk = {usable, tail_be32};
    const SelCall sc = {n_sel_handles, sel_handles, sel_index};
    return rows_lookup_sum(ctx, UINT32_MAX, n_input_handles, input_handles, n_table_handles, table_handles, mult_handle, n_lookups,
                           width, theta_be32, beta_be32, out_commitment48, out_closing32, out_handle, &zk, &sc);
}
int kzg_rows_commit_multiplicities(kzg_ctx* ctx, uint32_t n_input_handles, const uint64_t* input_handles,
                                   uint32_t n_table_handles, const uint64_t* table_handles, uint32_t n_lookups, uint32_t width,
                                   uint8_t out_commitment48[48], uint64_t* out_missing, uint64_t* out_handle) {
    return rows_multiplicities(ctx, UINT32_MAX, n_input_handles, input_handles, n_table_handles, table_handles, n_lookups, width,
                               out_commitment48, out_missing, out_handle, nullptr, nullptr);
}
int kzg_rows_commit_multiplicities_zk(kzg_ctx* ctx, uint32_t n_input_handles, const uint64_t* input_handles,
                                      uint32_t n_table_handles, const uint64_t* table_handles, uint32_t n_lookups, uint32_t width,
                                      uint64_t usable, const uint8_t* tail_be32, uint8_t out_commitment48[48],
                                      uint64_t* out_missing, uint64_t* out_handle) {
    const Blind zk = {usable, tail_be32};
    return rows_multiplicities(ctx, UINT32_MAX, n_input_handles, input_handles, n_table_handles, table_handles, n_lookups, width,
                               out_commitment48, out_missing, out_handle, &zk, nullptr);
}
int kzg_rows_commit_multiplicities_sel(kzg_ctx* ctx, uint32_t n_input_handles, const uint64_t* input_handles,
                                       uint32_t n_table_handles, const uint64_t* table_handles, uint32_t n_sel_handles,
                                       const uint64_t* sel_handles, const uint32_t* sel_index, uint32_t n_lookups, uint32_t width,
                                       uint64_t usable, const uint8_t* tail_be32, uint8_t out_commitment48[48],
                                       uint64_t* out_missing, uint64_t* out_handle) {
    const Blind zk = {usable, tail_be32};
    const SelCall sc = {n_sel_handles, sel_handles, sel_index};
    return rows_multiplicities(ctx, UINT32_MAX, n_input_handles, input_handles, n_table_handles, table_handles, n_lookups, width,
                               out_commitment48, out_missing, out_handle, &zk, &sc);
}
// the same with every rotation 0 and no lookup part
int kzg_rows_commit_quotient(kzg_ctx* ctx, uint32_t n_handles, const uint64_t* handles, const kzg_quotient_gate* gate,
                             const kzg_quotient_perm* perm, uint32_t ext_log, uint32_t n_pieces, uint8_t* out_commitments48,
                             uint64_t* out_handle) {
    if (!gate) return KZG_E_ARG;
    const kzg_quotient_terms terms = quotient_plain_terms(gate);
    return rows_quotient(ctx, UINT32_MAX, n_handles, handles, &terms, perm, nullptr, nullptr, nullptr, ext_log, n_pieces,
                         out_commitments48, out_handle, true);
}
int kzg_rows_commit_quotient_ext(kzg_ctx* ctx, uint32_t n_handles, const uint64_t* handles, const kzg_quotient_terms* gate,
                                 const kzg_quotient_perm* perm, const kzg_quotient_lookup* lookup, uint32_t ext_log,
                                 uint32_t n_pieces, uint8_t* out_commitments48, uint64_t* out_handle) {
    return rows_quotient(ctx, UINT32_MAX, n_handles, handles, gate, perm, lookup, nullptr, nullptr, ext_log, n_pieces,
                         out_commitments48, out_handle, false);
}
// active == NULL is kzg_rows_commit_quotient_ext
int kzg_rows_commit_quotient_zk(kzg_ctx* ctx, uint32_t n_handles, const uint64_t* handles, const kzg_quotient_terms* gate,
                                const kzg_quotient_perm* perm, const kzg_quotient_lookup* lookup,
                                const kzg_quotient_active* active, uint32_t ext_log, uint32_t n_pieces,
                                uint8_t* out_commitments48, uint64_t* out_handle) {
    return rows_quotient(ctx, UINT32_MAX, n_handles, handles, gate, perm, lookup, nullptr, active, ext_log, n_pieces,
                         out_commitments48, out_handle, false);
}
// selectors == NULL is kzg_rows_commit_quotient_zk
int kzg_rows_commit_quotient_sel(kzg_ctx* ctx, uint32_t n_handles, const uint64_t* handles, const kzg_quotient_terms* gate,
                                 const kzg_quotient_perm* perm, const kzg_quotient_lookup* lookup,
                                 const kzg_quotient_selectors* selectors, const kzg_quotient_active* active, uint32_t ext_log,
                                 uint32_t n_pieces, uint8_t* out_commitments48, uint64_t* out_handle) {
    return rows_quotient(ctx, UINT32_MAX, n_handles, handles, gate, perm, lookup, selectors, active, ext_log, n_pieces,
                         out_commitments48, out_handle, false);
}
int kzg_rows_quotient_part(kzg_ctx* ctx, uint32_t n_handles, const uint64_t* handles, const kzg_quotient_terms* gate,
                           const kzg_quotient_perm* perm, const kzg_quotient_link* link, const kzg_quotient_lookup* lookup,
                           const kzg_quotient_active* active, uint32_t ext_log, const uint8_t* scale_be32, uint64_t* inout_acc) {
    return rows_quotient_part(ctx, UINT32_MAX, n_handles, handles, gate, perm, link, lookup, nullptr, active, ext_log, scale_be32,
                              inout_acc);
}
int kzg_rows_quotient_part_sel(kzg_ctx* ctx, uint32_t n_handles, const uint64_t* handles, const kzg_quotient_terms* gate,
                               const kzg_quotient_perm* perm, const kzg_quotient_link* link, const kzg_quotient_lookup* lookup,
                               const kzg_quotient_selectors* selectors, const kzg_quotient_active* active, uint32_t ext_log,
                               const uint8_t* scale_be32, uint64_t* inout_acc) {
    return rows_quotient_part(ctx, UINT32_MAX, n_handles, handles, gate, perm, link, lookup, selectors, active, ext_log,
                              scale_be32, inout_acc);
}
int kzg_rows_quotient_finish(kzg_ctx* ctx, uint64_t acc, uint32_t n_pieces, uint8_t* out_commitments48, uint64_t* out_handle) {
    return rows_quotient_finish(ctx, UINT32_MAX, acc, n_pieces, out_commitments48, out_handle);
}
int kzg_rows_release(kzg_ctx* ctx, uint64_t handle) { return rows_release(ctx, UINT32_MAX, handle); }
int kzg_rows_stats(kzg_ctx* ctx, uint64_t out_live_sets_bytes[2]) {
    if (!ctx || !out_live_sets_bytes) return KZG_E_ARG;
    std::lock_guard<std::mutex> lk(ctx->sets_mu);
    uint64_t n = 0, bytes = 0;
    for (const auto& kv : ctx->sets)
        if (!kv.second.released) {
            n++;
            bytes += kv.second.buf.cap;
        }
    out_live_sets_bytes[0] = n;
    out_live_sets_bytes[1] = bytes;
    return KZG_OK;
}

}  // extern "C"
