// abi_test.hip -- test hooks of the library (include/kzg_mi355x_test.h): single field / group operations on the GPU and
// the host-side point encoder, so that tests/ can compare each of them with the oracle.  Not part of the serving surface.
#include "ctx.hip.h"

using namespace kzg_impl;

namespace {

// ---- unit-op test kernels
// Fr: saturated 32-bit Montgomery (field.hip.h).  Fp: op 0 mul / 1 add / 2 sub / 4 sqr on the 28-bit-limb working
// representation (fp28.hip.h); op 3 = the plain-C++ 12 x 32-bit CIOS reference product.
__global__ void __launch_bounds__(256) k_test_fr(int op, const uint8_t* a_be, const uint8_t* b_be, uint8_t* out_be,
                                                  uint64_t n) {
    uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    if (op == 3) {  // the saturated 8 x 32-bit CIOS reference (field.hip.h), self-contained
        fr_t a, b, r;
        limbs_from_be<8>(a.l, a_be + 32 * j);
        limbs_from_be<8>(b.l, b_be + 32 * j);
        f_to_mont(a, a);
        f_to_mont(b, b);
        f_mul_inline(r, a, b);
        f_from_mont(r, r);
        limbs_to_be<8>(out_be + 32 * j, r.l);
        return;
    }
    uint32_t wa[8], wb[8], wr[8];
    limbs_from_be<8>(wa, a_be + 32 * j);
    limbs_from_be<8>(wb, b_be + 32 * j);
    fr9_t a, b, r;
    fr9_from_words(a, wa);
    fr9_from_words(b, wb);
    fr9_to_mont(a, a);
    fr9_to_mont(b, b);
    if (op == 0) fr9_mul(r, a, b);
    else if (op == 1) fr9_add(r, a, b);
    else if (op == 2) fr9_sub4(r, a, b);
    else if (op == 5 || op == 6) {
        // k (a + b) summed lazily, k = 1 + (a mod 29) <= 29: a value up to 58 r with limbs up to 2^30.9, then the
        // product-free reductions: 5 = fr9_reduce (canonical), 6 = fr9_reduce_approx alone (< 2r)
        const uint32_t k = 1u + (uint32_t)((((uint64_t)wa[1] << 32) | wa[0]) % 29u);   // test side: (a mod 2^64) mod 29
        fr9_t s;
        fr9_add(s, a, b);
        r = s;
        for (uint32_t i = 1; i < k; i++) {
            fr9_add(r, r, s);
            if ((i & 1) == 0) fr9_norm(r, r);        // limbs stay below 2^31
        }
        if (op == 5) fr9_reduce(r, r);
        else {
            fr9_norm(r, r);
            fr9_reduce_approx(r, r);
        }
    }
    else fr9_mul(r, a, a);
    fr9_from_mont(r, r);
    fr9_to_words(wr, r);
    limbs_to_be<8>(out_be + 32 * j, wr);
}
__global__ void __launch_bounds__(256) k_test_fp(int op, const uint8_t* a_be, const uint8_t* b_be, uint8_t* out_be,
                                                  uint64_t n) {
    uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    if (op == 3) {
        fp32_t a, b, r;
        limbs_from_be<12>(a.l, a_be + 48 * j);
        limbs_from_be<12>(b.l, b_be + 48 * j);
        f_to_mont(a, a);
        f_to_mont(b, b);
        f_mul_inline(r, a, b);
        f_from_mont(r, r);
        limbs_to_be<12>(out_be + 48 * j, r.l);
        return;
    }
    fp_t a, b, r;
    fp_from_be48(a, a_be + 48 * j);
    fp_from_be48(b, b_be + 48 * j);
    if (op == 0) fp_mul(r, a, b);
    else if (op == 1) fp_add(r, a, b);
    else if (op == 2) fp_sub4(r, a, b);
    else fp_sqr(r, a);
    fp_to_be48(out_be + 48 * j, r);
}
__global__ void __launch_bounds__(256) k_test_g1(int op, const uint8_t* a_be, const uint8_t* b_be, uint8_t* out_be,
                                                  uint64_t n) {
    uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    g1_aff28 a, b, o;
    fp_from_be48(a.x, a_be + 96 * j); fp_from_be48(a.y, a_be + 96 * j + 48);
    fp_from_be48(b.x, b_be + 96 * j); fp_from_be48(b.y, b_be + 96 * j + 48);
    g1_xyzz_t pa, pb, r, t;
    g1_from_aff(pa, a);
    g1_from_aff(pb, b);
    if (op == 0) { r = pa; g1_madd_checked(r, b); }
    else if (op == 1) { g1_dbl(t, pa); g1_add(r, t, pb); }
    else if (op == 2) { g1_dbl(r, pa); }
    else if (op == 3) { g1_dbl(t, pa); g1_dbl(r, t); }
    else {  // long dependent chain: ((a + b) + b + ... ) exercising the class invariants across many mixed adds
        r = pa;
        for (int k = 0; k < 40; k++) g1_madd_checked<true>(r, (k & 1) ? a : b);  // the inlined-product variant
    }
    g1_to_aff(o, r);
    fp_to_be48(out_be + 96 * j, o.x);
    fp_to_be48(out_be + 96 * j + 48, o.y);
}

// lane-parallel point operations (fp_lp.hip.h), one wave per element: op 5 = 2a + b (full addition of two XYZZ points),
// 6 = 2 * (2a), 7 = ten rounds of r <- 2r + b starting from a (class invariants across a long dependent chain)
__global__ void __launch_bounds__(64) k_test_g1_lp(int op, const uint8_t* a_be, const uint8_t* b_be, uint8_t* out_be) {
    __shared__ LpScratch sm;
    __shared__ g1_xyzz_t pa, pb, r;
    const uint64_t j = blockIdx.x;
    const LpLane k = lp_lane();
    if (threadIdx.x == 0) {
        g1_aff28 a, b;
        fp_from_be48(a.x, a_be + 96 * j); fp_from_be48(a.y, a_be + 96 * j + 48);
        fp_from_be48(b.x, b_be + 96 * j); fp_from_be48(b.y, b_be + 96 * j + 48);
        g1_xyzz_t ta, tb, t2;
        g1_from_aff(ta, a);
        g1_from_aff(tb, b);
        g1_dbl(t2, ta);
        store_xyzz(&pa, op == 7 ? ta : t2);
        store_xyzz(&pb, tb);
    }
    __syncthreads();
    if (op == 5) lp_add(sm, &r, &pa, &pb, k);
    else if (op == 6) lp_dbl(sm, &r, &pa, k);
    else {
        for (int it = 0; it < 10; it++) {
            lp_dbl(sm, &pa, &pa, k);
            lp_add(sm, &pa, &pa, &pb, k);
        }
        if (threadIdx.x < 56) reinterpret_cast<uint32_t*>(&r)[threadIdx.x] = reinterpret_cast<uint32_t*>(&pa)[threadIdx.x];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        g1_xyzz_t v;
        load_xyzz(v, &r);
        g1_aff28 o;
        g1_to_aff(o, v);
        fp_to_be48(out_be + 96 * j, o.x);
        fp_to_be48(out_be + 96 * j + 48, o.y);
    }
}

// ---- raw-limb test kernels (kzg_test_fp_raw / kzg_test_g1_raw): limbs in as they are, limbs out as they are -- no conversion,
// no Montgomery entry or exit, no canonicalisation beyond what the operation under test does itself, so that tests/ can put every
// operand on the bounds of its representation class (tests/fp28_ref.py) and compare every output limb
KZG_DEV void fp_ld_raw(fp_t& r, const uint32_t* p) {
#pragma unroll
    for (int i = 0; i < 14; i++) r.l[i] = p[i];
}
template <int OP>
__global__ void __launch_bounds__(256) k_test_fp_raw(const uint32_t* a_l, const uint32_t* b_l, const uint32_t* c_l,
                                                      const uint32_t* d_l, uint32_t* out, uint64_t n) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    fp_t a, b, r;
    fp_ld_raw(a, a_l + 14 * j);
    fp_ld_raw(b, b_l + 14 * j);
    if constexpr (OP == 0) fp_mul(r, a, b);
    else if constexpr (OP == 1) fp_mul_inline(r, a, b);
    else if constexpr (OP == 2) fp_sqr(r, a);
    else if constexpr (OP == 3) fp_sqr_inline(r, a);
    else if constexpr (OP == 4) {
        fp_t c, d;
        fp_ld_raw(c, c_l + 14 * j);
        fp_ld_raw(d, d_l + 14 * j);
        fp_mul2_inline(r, a, b, c, d);
    }
    else if constexpr (OP == 5) { fp_sub4(r, a, b); fp_norm(r, r); }
    else if constexpr (OP == 6) { fp_sub8(r, a, b); fp_norm(r, r); }
    else if constexpr (OP == 7) { fp_sub16(r, a, b); fp_norm(r, r); }
    else if constexpr (OP == 8) fp_neg8(r, a);
    else if constexpr (OP == 9) fp_canon(r, a);
    else if constexpr (OP == 10) fp_canon_mont(r, a);
    else if constexpr (OP == 11) fp_neg_canon(r, a);
    else {
        fp_zero(r);
        r.l[0] = fp_is_zero_n(a) ? 1u : 0u;
    }
#pragma unroll
    for (int i = 0; i < 14; i++) out[14 * j + i] = r.l[i];
}
// lane-parallel forms: four independent elements per wave, one per DPP row (element 4 * block + row); rows past n run on zeros.
// op 13 = lp_mul, 14 = lp_norm on the 64-bit lane values a (low words) | b (high words) << 32
__global__ void __launch_bounds__(64) k_test_lp_raw(int op, const uint32_t* a_l, const uint32_t* b_l, uint32_t* out, uint64_t n) {
    const LpLane k = lp_lane();
    const uint64_t e = 4ull * blockIdx.x + k.row;
    const bool live = e < n && k.j < 14;
    const uint32_t x = live ? a_l[14 * e + k.j] : 0u, y = live ? b_l[14 * e + k.j] : 0u;
    const uint32_t r = op == 13 ? lp_mul(x, y, k) : lp_norm((uint64_t)x | ((uint64_t)y << 32), k);
    if (live) out[14 * e + k.j] = r;
}
__global__ void __launch_bounds__(256) k_test_fr_raw(int op, const uint32_t* a_l, const uint32_t* b_l, uint32_t* out, uint64_t n) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    fr9_t a, b, r;
#pragma unroll
    for (int i = 0; i < 9; i++) { a.l[i] = a_l[9 * j + i]; b.l[i] = b_l[9 * j + i]; }
    if (op == 0) fr9_mul(r, a, b);
    else if (op == 1) fr9_sub4(r, a, b);
    else if (op == 2) fr9_sub8(r, a, b);
    else if (op == 3) fr9_norm(r, a);
    else if (op == 4) fr9_reduce(r, a);
    else fr9_reduce_approx(r, a);
#pragma unroll
    for (int i = 0; i < 9; i++) out[9 * j + i] = r.l[i];
}
// points on raw XYZZ limbs (4 x 14 words per operand; the mixed additions read b's first 28 words as the affine x, y); the result
// leaves as the affine point, 96 big-endian bytes.  OP 0 / 1 = g1_add<false / true>, 2 / 3 = g1_madd<false / true>, 4 = g1_dbl
KZG_DEV void xyzz_ld_raw(g1_xyzz_t& p, const uint32_t* w) {
    fp_ld_raw(p.x, w); fp_ld_raw(p.y, w + 14); fp_ld_raw(p.zz, w + 28); fp_ld_raw(p.zzz, w + 42);
}
template <int OP>
__global__ void __launch_bounds__(64) k_test_g1_raw(const uint32_t* a_l, const uint32_t* b_l, uint8_t* out_be, uint64_t n) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    g1_xyzz_t pa, pb, r;
    xyzz_ld_raw(pa, a_l + 56 * j);
    xyzz_ld_raw(pb, b_l + 56 * j);
    if constexpr (OP == 0) g1_add<false>(r, pa, pb);
    else if constexpr (OP == 1) g1_add<true>(r, pa, pb);
    else if constexpr (OP == 2 || OP == 3) {
        g1_aff28 q;
        q.x = pb.x; q.y = pb.y;
        r = pa;
        g1_madd_checked<OP == 3>(r, q);
    }
    else g1_dbl(r, pa);
    g1_aff28 o;
    g1_to_aff(o, r);
    fp_to_be48(out_be + 96 * j, o.x);
    fp_to_be48(out_be + 96 * j + 48, o.y);
}
// op 5 = lp_add, 6 = lp_dbl: one wave per element
__global__ void __launch_bounds__(64) k_test_g1_lp_raw(int op, const uint32_t* a_l, const uint32_t* b_l, uint8_t* out_be) {
    __shared__ LpScratch sm;
    __shared__ g1_xyzz_t pa, pb, r;
    const uint64_t j = blockIdx.x;
    const LpLane k = lp_lane();
    if (threadIdx.x < 56) {
        reinterpret_cast<uint32_t*>(&pa)[threadIdx.x] = a_l[56 * j + threadIdx.x];
        reinterpret_cast<uint32_t*>(&pb)[threadIdx.x] = b_l[56 * j + threadIdx.x];
    }
    __syncthreads();
    if (op == 5) lp_add(sm, &r, &pa, &pb, k);
    else lp_dbl(sm, &r, &pa, k);
    __syncthreads();
    if (threadIdx.x == 0) {
        g1_xyzz_t v;
        load_xyzz(v, &r);
        g1_aff28 o;
        g1_to_aff(o, v);
        fp_to_be48(out_be + 96 * j, o.x);
        fp_to_be48(out_be + 96 * j + 48, o.y);
    }
}

}  // namespace

extern "C" {

// dev-only prototype hooks (scripts/proto/): compiled in only by `KZG_WITH_PROTO=1 python -m zkp_subnet_amd.build`;
// the shipped library and include/kzg_mi355x.h do not carry them
#ifdef KZG_WITH_PROTO
#include "../../scripts/proto/baff_hook.inc"
#endif

// test hooks for the host-side encoder (finish_host.cpp): no GPU involved
int kzg_host_xyzz_to_c48(const uint32_t xyzz_limbs28[56], uint8_t out48[48]) {
    if (!xyzz_limbs28 || !out48) return KZG_E_ARG;
    kzg_host::xyzz_to_c48(xyzz_limbs28, out48);
    return KZG_OK;
}
int kzg_host_xyzz_pair_to_c48(const uint32_t a_limbs28[56], const uint32_t b_limbs28[56], uint8_t out_a48[48],
                              uint8_t out_b48[48]) {
    if (!a_limbs28 || !b_limbs28 || !out_a48 || !out_b48) return KZG_E_ARG;
    kzg_host::xyzz_pair_to_c48(a_limbs28, b_limbs28, out_a48, out_b48);
    return KZG_OK;
}
int kzg_host_xyzz_to_partial192(const uint32_t xyzz_limbs28[56], uint8_t out192[192]) {
    if (!xyzz_limbs28 || !out192) return KZG_E_ARG;
    kzg_host::xyzz_to_partial192(xyzz_limbs28, out192);
    return KZG_OK;
}

int kzg_test_field(kzg_ctx* ctx, int field, int op, const uint8_t* a_be, const uint8_t* b_be, uint8_t* out_be,
                   uint64_t n) {
    if (!ctx || !a_be || !b_be || !out_be || !n) return KZG_E_ARG;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    LaneHold H(ctx);
    if (int rc = H.take()) return rc;
    Lane& L = H.L();
    const size_t w = field == 0 ? 48 : 32;
    HIPCHK(ctx, L.in_be.ensure(2 * n * w));
    HIPCHK(ctx, L.out_be.ensure(n * w));
    uint8_t* da = L.in_be.as<uint8_t>();
    uint8_t* db = da + n * w;
    HIPCHK(ctx, hipMemcpyAsync(da, a_be, n * w, hipMemcpyHostToDevice, L.stream));
    HIPCHK(ctx, hipMemcpyAsync(db, b_be, n * w, hipMemcpyHostToDevice, L.stream));
    uint32_t blocks = (uint32_t)((n + 255) / 256);
    if (field == 0) k_test_fp<<<blocks, 256, 0, L.stream>>>(op, da, db, L.out_be.as<uint8_t>(), n);
    else if (op == 7 || op == 8) launch_fr_inv_test(L.stream, da, L.out_be.as<uint8_t>(), n, op == 8);   // the device-side inversion alone
    else if (op == 9) {   // the batched inversion of kzg_rows_commit_lookup_sum alone: n elements, one fr9_inv
        HIPCHK(ctx, L.coeffA.ensure(n * 32));
        HIPCHK(ctx, L.coeffB.ensure(n * 32));
        HIPCHK(ctx, L.hbuf.ensure(poly_level_words(n) * 4));
        HIPCHK(ctx, L.hnext.ensure(poly_level_words(n) * 4));
        HIPCHK(ctx, L.scal.ensure(64));   // [0, 32) the scan's closing slot (unused), [32] zero flag, [36] range flag (unused)
        uint32_t* q = L.coeffA.as<uint32_t>();
        uint32_t* fl = L.scal.as<uint32_t>();
        HIPCHK(ctx, hipMemsetAsync(fl, 0, 64, L.stream));
        launch_fr_from_be(L.stream, da, q, n, 1, fl + 9);
        launch_fr_batch_inv(L.stream, q, L.coeffB.as<uint32_t>(), nullptr, L.coeffB.as<uint32_t>(), n, L.hbuf.as<uint32_t>(),
                            L.hnext.as<uint32_t>(), L.scal.as<uint8_t>(), fl + 8);
        launch_fr_to_be(L.stream, L.coeffB.as<uint32_t>(), L.out_be.as<uint8_t>(), n, 1);
        uint32_t zf = 0;
        HIPCHK(ctx, hipMemcpyAsync(&zf, fl + 8, 4, hipMemcpyDeviceToHost, L.stream));
        HIPCHK(ctx, hipMemcpyAsync(out_be, L.out_be.p, n * w, hipMemcpyDeviceToHost, L.stream));
        HIPCHK(ctx, hipStreamSynchronize(L.stream));
        HIPCHK(ctx, hipGetLastError());
        H.clean = true;
        if (zf) return fail(ctx, KZG_E_ARG, "batched inversion: an element is zero");
        return KZG_OK;
    }
    else k_test_fr<<<blocks, 256, 0, L.stream>>>(op, da, db, L.out_be.as<uint8_t>(), n);
    HIPCHK(ctx, hipMemcpyAsync(out_be, L.out_be.p, n * w, hipMemcpyDeviceToHost, L.stream));
    HIPCHK(ctx, hipStreamSynchronize(L.stream));
    HIPCHK(ctx, hipGetLastError());
    H.clean = true;
    return KZG_OK;
}
int kzg_test_g1(kzg_ctx* ctx, int op, const uint8_t* a_be96, const uint8_t* b_be96, uint8_t* out_be96, uint64_t n) {
    if (!ctx || !a_be96 || !b_be96 || !out_be96 || !n) return KZG_E_ARG;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    LaneHold H(ctx);
    if (int rc = H.take()) return rc;
    Lane& L = H.L();
    HIPCHK(ctx, L.in_be.ensure(2 * n * 96));
    HIPCHK(ctx, L.out_be.ensure(n * 96));
    uint8_t* da = L.in_be.as<uint8_t>();
    uint8_t* db = da + n * 96;
    HIPCHK(ctx, hipMemcpyAsync(da, a_be96, n * 96, hipMemcpyHostToDevice, L.stream));
    HIPCHK(ctx, hipMemcpyAsync(db, b_be96, n * 96, hipMemcpyHostToDevice, L.stream));
    if (op >= 5) k_test_g1_lp<<<(uint32_t)n, 64, 0, L.stream>>>(op, da, db, L.out_be.as<uint8_t>());
    else k_test_g1<<<(uint32_t)((n + 255) / 256), 256, 0, L.stream>>>(op, da, db, L.out_be.as<uint8_t>(), n);
    HIPCHK(ctx, hipMemcpyAsync(out_be96, L.out_be.p, n * 96, hipMemcpyDeviceToHost, L.stream));
    HIPCHK(ctx, hipStreamSynchronize(L.stream));
    HIPCHK(ctx, hipGetLastError());
    H.clean = true;
    return KZG_OK;
}

#define KZG_RAW_MAX_N (1ull << 22)   // elements per raw-hook call (tests pass a few thousand)
int kzg_test_fp_raw(kzg_ctx* ctx, int field, int op, const uint32_t* a, const uint32_t* b, const uint32_t* c, const uint32_t* d,
                    uint32_t* out, uint64_t n) {
    if (!ctx || !a || !out || !n || n > KZG_RAW_MAX_N || (field != 0 && field != 1) || op < 0 || op > (field == 0 ? 14 : 5))
        return KZG_E_ARG;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    LaneHold H(ctx);
    if (int rc = H.take()) return rc;
    Lane& L = H.L();
    const size_t bytes = n * (field == 0 ? 14 : 9) * sizeof(uint32_t);
    HIPCHK(ctx, L.in_be.ensure(4 * bytes));
    HIPCHK(ctx, L.out_be.ensure(bytes));
    const uint32_t* src[4] = {a, b ? b : a, c ? c : a, d ? d : a};     // an operand the operation does not read may be NULL
    uint32_t* dv[4];
    for (int i = 0; i < 4; i++) {
        dv[i] = reinterpret_cast<uint32_t*>(L.in_be.as<uint8_t>() + i * bytes);
        HIPCHK(ctx, hipMemcpyAsync(dv[i], src[i], bytes, hipMemcpyHostToDevice, L.stream));
    }
    uint32_t* dout = L.out_be.as<uint32_t>();
    const uint32_t blocks = (uint32_t)((n + 255) / 256);
    if (field == 1) k_test_fr_raw<<<blocks, 256, 0, L.stream>>>(op, dv[0], dv[1], dout, n);
    else if (op >= 13) k_test_lp_raw<<<(uint32_t)((n + 3) / 4), 64, 0, L.stream>>>(op, dv[0], dv[1], dout, n);
    else {
        switch (op) {
#define FP_RAW_CASE(OP) case OP: k_test_fp_raw<OP><<<blocks, 256, 0, L.stream>>>(dv[0], dv[1], dv[2], dv[3], dout, n); break;
            FP_RAW_CASE(0) FP_RAW_CASE(1) FP_RAW_CASE(2) FP_RAW_CASE(3) FP_RAW_CASE(4) FP_RAW_CASE(5) FP_RAW_CASE(6)
            FP_RAW_CASE(7) FP_RAW_CASE(8) FP_RAW_CASE(9) FP_RAW_CASE(10) FP_RAW_CASE(11) FP_RAW_CASE(12)
#undef FP_RAW_CASE
        }
    }
    HIPCHK(ctx, hipMemcpyAsync(out, dout, bytes, hipMemcpyDeviceToHost, L.stream));
    HIPCHK(ctx, hipStreamSynchronize(L.stream));
    HIPCHK(ctx, hipGetLastError());
    H.clean = true;
    return KZG_OK;
}
int kzg_test_g1_raw(kzg_ctx* ctx, int op, const uint32_t* a_xyzz, const uint32_t* b_xyzz, uint8_t* out_be96, uint64_t n) {
    if (!ctx || !a_xyzz || !out_be96 || !n || n > KZG_RAW_MAX_N || op < 0 || op > 6) return KZG_E_ARG;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    LaneHold H(ctx);
    if (int rc = H.take()) return rc;
    Lane& L = H.L();
    const size_t bytes = n * 56 * sizeof(uint32_t);
    HIPCHK(ctx, L.in_be.ensure(2 * bytes));
    HIPCHK(ctx, L.out_be.ensure(n * 96));
    uint32_t* da = L.in_be.as<uint32_t>();
    uint32_t* db = da + n * 56;
    HIPCHK(ctx, hipMemcpyAsync(da, a_xyzz, bytes, hipMemcpyHostToDevice, L.stream));
    HIPCHK(ctx, hipMemcpyAsync(db, b_xyzz ? b_xyzz : a_xyzz, bytes, hipMemcpyHostToDevice, L.stream));   // the doublings read no b
    uint8_t* dout = L.out_be.as<uint8_t>();
    const uint32_t blocks = (uint32_t)((n + 63) / 64);
    switch (op) {
        case 0: k_test_g1_raw<0><<<blocks, 64, 0, L.stream>>>(da, db, dout, n); break;
        case 1: k_test_g1_raw<1><<<blocks, 64, 0, L.stream>>>(da, db, dout, n); break;
        case 2: k_test_g1_raw<2><<<blocks, 64, 0, L.stream>>>(da, db, dout, n); break;
        case 3: k_test_g1_raw<3><<<blocks, 64, 0, L.stream>>>(da, db, dout, n); break;
        case 4: k_test_g1_raw<4><<<blocks, 64, 0, L.stream>>>(da, db, dout, n); break;
        default: k_test_g1_lp_raw<<<(uint32_t)n, 64, 0, L.stream>>>(op, da, db, dout); break;
    }
    HIPCHK(ctx, hipMemcpyAsync(out_be96, dout, n * 96, hipMemcpyDeviceToHost, L.stream));
    HIPCHK(ctx, hipStreamSynchronize(L.stream));
    HIPCHK(ctx, hipGetLastError());
    H.clean = true;
    return KZG_OK;
}

// ---- the NTT's pass plans (tests/test_ntt_plans_cpu.py, tests/test_gpu_ntt_plans.py)
int kzg_test_ntt_plan_of(int log_n, int kernel, int tile_log, int* out_S, int* out_logC, int* out_passes) {
    if (!out_S || !out_logC || !out_passes) return fail(nullptr, KZG_E_ARG, "ntt plan: null output");
    if (log_n < 1 || log_n > 31 || kernel < -1 || kernel > 1 || (tile_log != 0 && (tile_log < 8 || tile_log > 11)))
        return fail(nullptr, KZG_E_ARG, "ntt plan: log_n in [1, 31], kernel in {-1, 0, 1}, tile_log 0 or in [8, 11]");
    const NttPlan pl = ntt_plan_for(log_n, kernel, tile_log);
    for (int p = 0; p < pl.passes; p++) {
        out_S[p] = pl.S[p];
        out_logC[p] = pl.logC[p];
    }
    *out_passes = pl.passes;
    return pl.radix2;
}
#define KZG_TEST_NTT_MAX_LOG 22      // elements per plan-hook call (as KZG_RAW_MAX_N)
int kzg_test_ntt_run(kzg_ctx* ctx, uint8_t* inout_be32, int log_n, int inverse, int kernel, int passes, const int* S,
                     const int* logC) {
    // the plan is judged first, with no context and no device: nothing invalid reaches a kernel
    if (!S || !logC || passes < 1 || passes > NTT_MAX_PASSES) return fail(ctx, KZG_E_ARG, "ntt plan: number of passes outside [1, 8]");
    if (kernel != 0 && kernel != 1) return fail(ctx, KZG_E_ARG, "ntt plan: kernel must be 0 (register-blocked) or 1 (radix-2)");
    if (log_n < 1 || log_n > KZG_TEST_NTT_MAX_LOG) return fail(ctx, KZG_E_ARG, "ntt plan: log_n outside [1, 22]");
    NttPlan pl;
    memset(&pl, 0, sizeof pl);
    pl.radix2 = kernel;
    pl.passes = passes;
    for (int p = 0; p < passes; p++) {
        pl.S[p] = S[p];
        pl.logC[p] = logC[p];
    }
    if (const char* why = ntt_plan_invalid(log_n, pl)) return fail(ctx, KZG_E_ARG, why);
    if (!ctx || !inout_be32) return fail(ctx, KZG_E_ARG, "ntt plan: no context or no data");
    // from here on: kzg_ntt's path (serve.hip), with the caller's plan in place of the production one
    const uint64_t n = (uint64_t)1 << log_n;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    LaneHold H(ctx);
    if (int rc = H.take()) return rc;
    Lane& L = H.L();
    prof_begin(ctx, L);
    int rc = clear_flags(ctx, L);
    if (rc) return rc;
    HIPCHK(ctx, L.coeffA.ensure(n * 32));
    HIPCHK(ctx, L.coeffB.ensure(n * 32));
    HIPCHK(ctx, L.out_be.ensure(n * 32));
    rc = upload_fr(ctx, L, inout_be32, n, L.coeffA.as<uint32_t>(), 1);
    if (rc) return rc;
    uint32_t *tw = nullptr, *invn = nullptr;
    rc = ensure_twiddles(ctx, L, log_n, inverse, &tw, inverse ? &invn : nullptr);
    if (rc) return rc;
    HIPCHK(ctx, L.ntt_mid.ensure(n * 48));
    {
        Span sp(ctx, L, KZG_T_NTT);
        run_fr_ntt_plan(L.stream, L.coeffA.as<uint32_t>(), L.coeffB.as<uint32_t>(), log_n, tw, inverse ? invn : nullptr,
                        L.ntt_mid.as<uint32_t>(), pl);
    }
    launch_fr_to_be(L.stream, L.coeffB.as<uint32_t>(), L.out_be.as<uint8_t>(), n, 1);
    rc = finish(ctx, L);
    if (rc) return rc;
    HIPCHK(ctx, hipMemcpy(inout_be32, L.out_be.p, n * 32, hipMemcpyDeviceToHost));
    H.clean = true;
    return KZG_OK;
}

// ---- the opening scan's plans (tests/test_poly_plans_cpu.py, tests/test_gpu_poly_plans.py)
// all four parameters -1: the plan the launchers pick themselves; otherwise the caller's, every parameter taken as given
static const char* poly_plan_from(uint64_t n, int l0, int64_t scan_max, int scan_nt, int lds, PolyPlan* pl) {
    if (!n) return "poly plan: no coefficients";
    if (l0 == -1 && scan_max == -1 && scan_nt == -1 && lds == -1) *pl = poly_plan(n);
    else {
        if (lds != 0 && lds != 1) return "poly plan: lds must be 0 or 1";
        *pl = poly_plan_levels(n, l0, scan_max < 0 ? 0 : (uint64_t)scan_max, scan_nt, lds != 0);
    }
    return poly_plan_invalid(*pl, n);
}
int kzg_test_poly_plan_of(uint64_t n, int l0, int64_t scan_max, int scan_nt, int lds, int* out_K, int* out_l, int* out_sq,
                          uint64_t* out_n, uint64_t* out_off, int* out_scan_nt, int* out_lds) {
    if (!out_K || !out_l || !out_sq || !out_n || !out_off || !out_scan_nt || !out_lds)
        return fail(nullptr, KZG_E_ARG, "poly plan: null output");
    PolyPlan pl;
    if (const char* why = poly_plan_from(n, l0, scan_max, scan_nt, lds, &pl)) return fail(nullptr, KZG_E_ARG, why);
    for (int k = 0; k <= pl.K; k++) {
        out_l[k] = k < pl.K ? pl.l[k] : 0;    // (level K is the scan's: it folds nothing into a further level)
        out_sq[k] = pl.sq[k];
        out_n[k] = pl.n[k];
        out_off[k] = pl.off[k];
    }
    *out_K = pl.K;
    *out_scan_nt = pl.scan_nt;
    *out_lds = pl.lds;
    return KZG_OK;
}
#define KZG_TEST_POLY_MAX_N ((uint64_t)1 << 22)   // coefficients per plan-hook call, all rows together (as KZG_RAW_MAX_N)
int kzg_test_poly_run(kzg_ctx* ctx, int form, int l0, int64_t scan_max, int scan_nt, int lds, const uint8_t* f_be32, uint64_t n,
                      uint32_t rows, int f_mont, const uint8_t* pair_row, const uint8_t* pair_pt, uint32_t npairs,
                      const uint8_t* pts, const uint8_t* alphas_be32, uint32_t nalphas, uint8_t* out_y_be32,
                      uint32_t* out_q_words) {
    // the plan is judged first, with no context and no device: nothing invalid reaches a kernel
    PolyPlan pl;
    if (const char* why = poly_plan_from(n, l0, scan_max, scan_nt, lds, &pl)) return fail(ctx, KZG_E_ARG, why);
    if (form < 0 || form > 5) return fail(ctx, KZG_E_ARG, "poly run: form outside [0, 5]");
    const bool quot = form == 0 || form >= 4, pairs = form == 3, points = form >= 4;
    const uint32_t max_rows = form <= 1 ? 1 : points ? POLY_MAX_POINTS : POLY_MAX_ROWS;
    if (!rows || rows > max_rows || n > KZG_TEST_POLY_MAX_N / rows)
        return fail(ctx, KZG_E_ARG, "poly run: 1 row (forms 0, 1), up to 16 (2, 3) or 4 (4, 5), at most 2^22 coefficients in all");
    if (!nalphas || nalphas > (form <= 2 ? 1u : (uint32_t)POLY_MAX_POINTS) || (form == 4 && nalphas != rows))
        return fail(ctx, KZG_E_ARG, "poly run: one point (forms 0 - 2), up to 4 (3, 5), one per vector (4)");
    if (pairs) {
        if (!pair_row || !pair_pt || !npairs || npairs > POLY_MAX_PAIRS) return fail(ctx, KZG_E_ARG, "poly run: 1 .. 64 pairs");
        for (uint32_t y = 0; y < npairs; y++)
            if (pair_row[y] >= rows || pair_pt[y] >= nalphas || (y && pair_pt[y] < pair_pt[y - 1]))
                return fail(ctx, KZG_E_ARG, "poly run: a pair names no row or no point, or the pairs are not point-major");
    }
    if (form == 5) {
        if (!pts) return fail(ctx, KZG_E_ARG, "poly run: form 5 takes a map of points");
        for (uint32_t p = 0; p < rows; p++)
            if (pts[p] >= nalphas) return fail(ctx, KZG_E_ARG, "poly run: the map names no point");
    }
    if (!ctx || !f_be32 || !alphas_be32 || !out_y_be32 || (quot && !out_q_words))
        return fail(ctx, KZG_E_ARG, "poly run: no context or no data");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    LaneHold H(ctx);
    if (int rc = H.take()) return rc;
    Lane& L = H.L();
    prof_begin(ctx, L);
    int rc = clear_flags(ctx, L);
    if (rc) return rc;
    hipStream_t s = L.stream;
    const uint32_t nout = pairs ? npairs : rows;          // evaluations, and rows of level scratch
    const uint64_t hrow = poly_level_words(n);
    const uint64_t stride = pairs ? n + 3 : n;            // form 3: the rows lie apart and in descending order
    HIPCHK(ctx, L.coeffA.ensure(rows * stride * 32));
    HIPCHK(ctx, L.coeffB.ensure(rows * n * 32));
    HIPCHK(ctx, L.hbuf.ensure(nout * hrow * 4));
    HIPCHK(ctx, L.hnext.ensure(nout * hrow * 4));
    HIPCHK(ctx, L.scal.ensure(POLY_MAX_POINTS * 32 + POLY_MAX_PAIRS * 64));
    if (quot) HIPCHK(ctx, L.qbuf.ensure(rows * n * 32));
    uint32_t* f = pairs ? L.coeffB.as<uint32_t>() : L.coeffA.as<uint32_t>();
    uint32_t* alpha_m = L.scal.as<uint32_t>();                         // POLY_MAX_POINTS x 8 words
    uint32_t* y_m = alpha_m + POLY_MAX_POINTS * 8;                     // POLY_MAX_PAIRS x 8 words
    uint8_t* y_be = L.scal.as<uint8_t>() + POLY_MAX_POINTS * 32 + POLY_MAX_PAIRS * 32;
    rc = upload_fr(ctx, L, f_be32, rows * n, f, f_mont ? 0 : 1);
    if (rc) return rc;
    // whatever a kernel fails to write must show: the quotient and the suffix values start from a pattern that is no result
    HIPCHK(ctx, hipMemsetAsync(L.hnext.p, 0xa5, nout * hrow * 4, s));
    if (quot) HIPCHK(ctx, hipMemsetAsync(L.qbuf.p, 0xa5, rows * n * 32, s));
    uint32_t* h = L.hbuf.as<uint32_t>();
    uint32_t* hn = L.hnext.as<uint32_t>();
    uint32_t* q = L.qbuf.as<uint32_t>();
    {
        Span sp(ctx, L, KZG_T_POLY);
        if (form == 0) launch_poly_open(s, pl, f, n, alpha_m, h, hn, y_m, q, alphas_be32, L.flags(), y_be);
        else if (form == 1) {
            launch_fr_from_host32(s, alphas_be32, alpha_m, 1, L.flags());
            launch_poly_open(s, pl, f, n, alpha_m, h, hn, y_m, nullptr, nullptr, nullptr, y_be);
        } else if (form == 2) launch_poly_eval_rows(s, pl, f, n, rows, alpha_m, h, hn, hrow, y_m, alphas_be32, L.flags(), y_be);
        else if (form == 3) {
            RowTab rt;
            memset(&rt, 0, sizeof rt);
            PairArg pa;
            memset(&pa, 0, sizeof pa);
            for (uint32_t j = 0; j < rows; j++) {
                uint32_t* dst = L.coeffA.as<uint32_t>() + (uint64_t)(rows - 1 - j) * stride * 8;
                HIPCHK(ctx, hipMemcpyAsync(dst, f + (uint64_t)j * n * 8, n * 32, hipMemcpyDeviceToDevice, s));
                rt.r[j] = dst;
            }
            for (uint32_t p = 0; p < nalphas; p++) memcpy(pa.a[p].w, alphas_be32 + 32 * (size_t)p, 32);
            memcpy(pa.row, pair_row, npairs);
            memcpy(pa.pt, pair_pt, npairs);
            launch_poly_eval_pairs(s, pl, rt, n, npairs, pa, alpha_m, h, hn, hrow, y_m, L.flags(), y_be);
        } else {
            for (uint32_t p = 0; p < nalphas; p++)
                launch_fr_from_host32(s, alphas_be32 + 32 * (size_t)p, alpha_m + 8 * p, 1, L.flags());
            launch_poly_open_points(s, pl, f, n, rows, alpha_m, h, hn, hrow, y_m, q, y_be, form == 5 ? pts : nullptr, form == 5);
        }
    }
    rc = finish(ctx, L);
    if (rc) return rc;
    HIPCHK(ctx, hipMemcpy(out_y_be32, y_be, nout * 32, hipMemcpyDeviceToHost));
    if (quot) HIPCHK(ctx, hipMemcpy(out_q_words, q, rows * n * 32, hipMemcpyDeviceToHost));
    H.clean = true;
    return KZG_OK;
}

// ---- the recurrence scan's plans (tests/test_recurrence_cpu.py, tests/test_gpu_recur_plans.py)
// both parameters -1: the plan the launcher picks itself; otherwise the caller's, both taken as given
static const char* recur_plan_from(uint64_t n, int l0, int64_t top_max, RecurPlan* pl) {
    if (!n) return "recur plan: no rows";
    if (l0 == -1 && top_max == -1) *pl = recur_plan(n);
    else *pl = recur_plan_levels(n, l0, top_max < 0 ? 0 : (uint64_t)top_max);
    return recur_plan_invalid(*pl, n);
}
int kzg_test_recur_plan_of(uint64_t n, int l0, int64_t top_max, int* out_K, int* out_l, uint64_t* out_n, uint64_t* out_off) {
    if (!out_K || !out_l || !out_n || !out_off) return fail(nullptr, KZG_E_ARG, "recur plan: null output");
    RecurPlan pl;
    if (const char* why = recur_plan_from(n, l0, top_max, &pl)) return fail(nullptr, KZG_E_ARG, why);
    for (int k = 0; k <= pl.K; k++) {
        out_l[k] = k < pl.K ? pl.l[k] : 0;    // (level K is the top kernel's: it folds nothing into a further level)
        out_n[k] = pl.n[k];
        out_off[k] = pl.off[k];
    }
    *out_K = pl.K;
    return KZG_OK;
}
#define KZG_TEST_RECUR_MAX_N ((uint64_t)1 << 22)   // steps per plan-hook call (as KZG_TEST_POLY_MAX_N)
int kzg_test_recur_run(kzg_ctx* ctx, int l0, int64_t top_max, const uint8_t* a_be32, const uint8_t* b_be32,
                       const uint8_t start_be32[32], uint64_t n, uint8_t* out_v_be32, uint8_t* out_closing_be32) {
    // the plan is judged first, with no context and no device: nothing invalid reaches a kernel
    RecurPlan pl;
    if (const char* why = recur_plan_from(n, l0, top_max, &pl)) return fail(ctx, KZG_E_ARG, why);
    if (n > KZG_TEST_RECUR_MAX_N) return fail(ctx, KZG_E_ARG, "recur run: at most 2^22 steps");
    if (!ctx || !a_be32 || !b_be32 || !start_be32 || !out_v_be32 || !out_closing_be32)
        return fail(ctx, KZG_E_ARG, "recur run: no context or no data");
    static const uint8_t R_BE[32] = {0x73, 0xED, 0xA7, 0x53, 0x29, 0x9D, 0x7D, 0x48, 0x33, 0x39, 0xD8, 0x08, 0x09, 0xA1, 0xD8, 0x05,
                                     0x53, 0xBD, 0xA4, 0x02, 0xFF, 0xFE, 0x5B, 0xFE, 0xFF, 0xFF, 0xFF, 0xFF, 0x00, 0x00, 0x00, 0x01};
    if (memcmp(start_be32, R_BE, 32) >= 0)   // (the serving call checks its starts on the host too; the kernel takes them as canonical)
        return fail(ctx, KZG_E_ARG, "recur run: start must be canonical (< r)");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    LaneHold H(ctx);
    if (int rc = H.take()) return rc;
    Lane& L = H.L();
    prof_begin(ctx, L);
    int rc = clear_flags(ctx, L);
    if (rc) return rc;
    hipStream_t s = L.stream;
    HIPCHK(ctx, L.coeffA.ensure(n * 32));
    HIPCHK(ctx, L.coeffB.ensure(n * 32));
    HIPCHK(ctx, L.qbuf.ensure(n * 32));
    HIPCHK(ctx, L.hbuf.ensure(recur_level_elems(n) * 32));
    HIPCHK(ctx, L.hnext.ensure(recur_level_elems(n) * 32));
    HIPCHK(ctx, L.scal.ensure(64));
    HIPCHK(ctx, L.out_be.ensure(n * 32));
    uint32_t *a = L.coeffA.as<uint32_t>(), *b = L.coeffB.as<uint32_t>(), *v = L.qbuf.as<uint32_t>();
    rc = upload_fr(ctx, L, a_be32, n, a, 1);
    if (rc) return rc;
    rc = upload_fr(ctx, L, b_be32, n, b, 1);
    if (rc) return rc;
    // whatever a kernel fails to write must show: the values and the level scratch start from a pattern that is no result
    HIPCHK(ctx, hipMemsetAsync(L.qbuf.p, 0xff, n * 32, s));
    HIPCHK(ctx, hipMemsetAsync(L.hbuf.p, 0xff, recur_level_elems(n) * 32, s));
    HIPCHK(ctx, hipMemsetAsync(L.hnext.p, 0xff, recur_level_elems(n) * 32, s));
    {
        Span sp(ctx, L, KZG_T_POLY);
        launch_recur_scan(s, pl, a, b, n, L.hbuf.as<uint32_t>(), L.hnext.as<uint32_t>(), start_be32, v, L.scal.as<uint8_t>(), nullptr);
    }
    // the words as the kernels left them, taken out of Montgomery form WITHOUT a reduction check: an unwritten cell (all ones)
    // comes back as a value that no reference holds
    launch_fr_to_be(s, v, L.out_be.as<uint8_t>(), n, 1);
    rc = finish(ctx, L);
    if (rc) return rc;
    HIPCHK(ctx, hipMemcpy(out_v_be32, L.out_be.p, n * 32, hipMemcpyDeviceToHost));
    HIPCHK(ctx, hipMemcpy(out_closing_be32, L.scal.p, 32, hipMemcpyDeviceToHost));
    H.clean = true;
    return KZG_OK;
}

// ---- the product and the additive scan's plans (tests/test_scan_plans_cpu.py, tests/test_gpu_scan_plans.py, reference
// tests/scan_ref.py).  Both parameters -1: the plan the launchers pick themselves; otherwise the caller's, both taken as given
static const char* scan_plan_from(uint64_t n, int l0, int64_t top_max, ScanPlan* pl) {
    if (!n) return "scan plan: no elements";
    if (l0 == -1 && top_max == -1) *pl = scan_plan(n);
    else *pl = scan_plan_levels(n, l0, top_max < 0 ? 0 : (uint64_t)top_max);
    return scan_plan_invalid(*pl, n);
}
int kzg_test_scan_plan_of(uint64_t n, int l0, int64_t top_max, int* out_K, int* out_l, uint64_t* out_n, uint64_t* out_off) {
    if (!out_K || !out_l || !out_n || !out_off) return fail(nullptr, KZG_E_ARG, "scan plan: null output");
    ScanPlan pl;
    if (const char* why = scan_plan_from(n, l0, top_max, &pl)) return fail(nullptr, KZG_E_ARG, why);
    for (int k = 0; k <= pl.K; k++) {
        out_l[k] = k < pl.K ? pl.l[k] : 0;    // (level K is the top kernel's: it folds nothing into a further level)
        out_n[k] = pl.n[k];
        out_off[k] = pl.off[k];
    }
    *out_K = pl.K;
    return KZG_OK;
}
#define KZG_TEST_SCAN_MAX_N ((uint64_t)1 << 22)   // elements per plan-hook call (as KZG_TEST_RECUR_MAX_N)
int kzg_test_scan_run(kzg_ctx* ctx, int form, int l0, int64_t top_max, const uint8_t* a_be32, const uint8_t* b_be32,
                      const uint8_t* start_be32, uint64_t n, uint8_t* out_be32, uint8_t* out_closing_be32, uint32_t* out_zero_flag) {
    // the plan is judged first, with no context and no device: nothing invalid reaches a kernel
    ScanPlan pl;
    if (const char* why = scan_plan_from(n, l0, top_max, &pl)) return fail(ctx, KZG_E_ARG, why);
    if (n > KZG_TEST_SCAN_MAX_N) return fail(ctx, KZG_E_ARG, "scan run: at most 2^22 elements");
    if (form < 0 || form > 4)
        return fail(ctx, KZG_E_ARG, "scan run: form must be 0 (product), 1 (chained product), 2 (1 / a), 3 (b / a) or 4 (sum)");
    const bool has_b = form == 0 || form == 1 || form == 3;
    if (!ctx || !a_be32 || (has_b && !b_be32) || (form == 1 && !start_be32) || !out_be32 || !out_closing_be32 || !out_zero_flag)
        return fail(ctx, KZG_E_ARG, "scan run: no context or no data");
    if (form == 1) {   // (the chained grand product checks its start on the host too; k_gp_chain_start takes it as canonical, not 0)
        static const uint8_t R_BE[32] = {0x73, 0xED, 0xA7, 0x53, 0x29, 0x9D, 0x7D, 0x48, 0x33, 0x39, 0xD8, 0x08, 0x09, 0xA1, 0xD8, 0x05,
                                         0x53, 0xBD, 0xA4, 0x02, 0xFF, 0xFE, 0x5B, 0xFE, 0xFF, 0xFF, 0xFF, 0xFF, 0x00, 0x00, 0x00, 0x01};
        static const uint8_t ZERO32[32] = {};
        if (memcmp(start_be32, R_BE, 32) >= 0 || memcmp(start_be32, ZERO32, 32) == 0)
            return fail(ctx, KZG_E_ARG, "scan run: start must be a canonical scalar (< r) other than 0");
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    LaneHold H(ctx);
    if (int rc = H.take()) return rc;
    Lane& L = H.L();
    prof_begin(ctx, L);
    int rc = clear_flags(ctx, L);
    if (rc) return rc;
    hipStream_t s = L.stream;
    HIPCHK(ctx, L.coeffA.ensure(n * 32));
    HIPCHK(ctx, L.coeffB.ensure(n * 32));
    HIPCHK(ctx, L.qbuf.ensure(n * 32));
    HIPCHK(ctx, L.hbuf.ensure(scan_level_elems(n) * 32));
    HIPCHK(ctx, L.hnext.ensure(scan_level_elems(n) * 32));
    HIPCHK(ctx, L.scal.ensure(64));   // [0, 32) the scan's closing slot, [32] its zero flag
    HIPCHK(ctx, L.out_be.ensure(n * 32));
    uint32_t *a = L.coeffA.as<uint32_t>(), *b = L.coeffB.as<uint32_t>(), *w = L.qbuf.as<uint32_t>();
    uint32_t *hN = L.hbuf.as<uint32_t>(), *hD = L.hnext.as<uint32_t>();
    uint8_t* cl = L.scal.as<uint8_t>();
    uint32_t* zf = L.scal.as<uint32_t>() + 8;
    rc = upload_fr(ctx, L, a_be32, n, a, 1);
    if (rc) return rc;
    if (has_b) {
        rc = upload_fr(ctx, L, b_be32, n, b, 1);
        if (rc) return rc;
    }
    // whatever a kernel fails to write must show: W, the level scratch, the closing slot and the flag start from a pattern that
    // is no result
    HIPCHK(ctx, hipMemsetAsync(L.qbuf.p, 0xff, n * 32, s));
    HIPCHK(ctx, hipMemsetAsync(L.hbuf.p, 0xff, scan_level_elems(n) * 32, s));
    HIPCHK(ctx, hipMemsetAsync(L.hnext.p, 0xff, scan_level_elems(n) * 32, s));
    HIPCHK(ctx, hipMemsetAsync(L.scal.p, 0xff, 64, s));
    if (form == 4) HIPCHK(ctx, hipMemsetAsync(zf, 0, 4, s));   // (the additive scan has no flag)
    const uint32_t* out = nullptr;
    {
        Span sp(ctx, L, KZG_T_POLY);
        if (form == 0 || form == 1) {
            launch_gp_scan(s, pl, a, b, n, hN, hD, cl, zf, form == 1 ? start_be32 : nullptr);
            out = a;
        } else if (form == 2) {
            launch_fr_batch_inv(s, pl, a, w, nullptr, w, n, hN, hD, cl, zf);
            out = w;
        } else if (form == 3) {
            launch_fr_batch_inv(s, pl, a, w, b, b, n, hN, hD, cl, zf);
            out = b;
        } else {
            launch_lk_sum_scan(s, pl, a, n, hN, cl);
            out = a;
        }
    }
    // the words as the kernels left them, taken out of Montgomery form WITHOUT a reduction check: an unwritten cell (all ones)
    // comes back as a value that no reference holds
    launch_fr_to_be(s, out, L.out_be.as<uint8_t>(), n, 1);
    rc = finish(ctx, L);
    if (rc) return rc;
    uint8_t rec[36];
    HIPCHK(ctx, hipMemcpy(out_be32, L.out_be.p, n * 32, hipMemcpyDeviceToHost));
    HIPCHK(ctx, hipMemcpy(rec, L.scal.p, 36, hipMemcpyDeviceToHost));
    memcpy(out_closing_be32, rec, 32);
    memcpy(out_zero_flag, rec + 32, 4);
    H.clean = true;
    return KZG_OK;
}

// ---- the hash join alone (tests/test_join_cpu.py, tests/test_gpu_join.py, reference tests/join_ref.py)
#define KZG_TEST_JOIN_MAX 4096u      // rows and slots per join-hook call
static const char* join_args_invalid(int build, int walk, uint64_t T, uint64_t rows, uint32_t w, uint32_t n_pay, int index,
                                     uint32_t cap, bool has_sel) {
    if (build != 0 && build != 1) return "join: build must be 0 (launch_join_build) or 1 (launch_join_build_rows)";
    if (walk < 0 || walk > 3) return "join: walk must be 0 (probe), 1 (probe_rows), 2 (probe_sel) or 3 (fetch)";
    if (!T || T > KZG_TEST_JOIN_MAX) return "join: T outside [1, 2^12]";
    if (!rows || rows > T) return "join: rows outside [1, T]";
    if ((build == 0 || walk == 0) && rows != T) return "join: launch_join_build and launch_join_probe take every row, rows must be T";
    if (!cap || (cap & (cap - 1)) || cap < rows || cap > KZG_TEST_JOIN_MAX) return "join: cap must be a power of two in [rows, 2^12]";
    if (!w || n_pay > KZG_MAX_BATCH_OPEN || w + n_pay > KZG_MAX_BATCH_OPEN) return "join: w >= 1 and w + n_pay <= 16 table columns";
    if (index != 0 && index != 1) return "join: index must be 0 or 1";
    if (index && walk != 3) return "join: the index column goes with the fetch only";
    if (walk == 3 && n_pay + (uint32_t)index == 0) return "join: a fetch needs a payload column or the index";
    if (has_sel != (walk == 2)) return "join: a selector column goes with launch_join_probe_sel, and only with it";
    return nullptr;
}
int kzg_test_join(kzg_ctx* ctx, int build, int walk, const uint8_t* tab_be32, const uint8_t* in_be32, const uint8_t* sel_be32,
                  uint64_t T, uint64_t rows, uint32_t w, uint32_t n_pay, int index, uint32_t cap, uint32_t* out_slots,
                  uint32_t* out_home, uint32_t* out_cnt, uint8_t* out_fetch_be32, uint64_t* out_missing, uint64_t* out_first,
                  uint32_t* out_overrun) {
    // the arguments are judged first, with no context and no device: nothing invalid reaches a kernel
    if (const char* why = join_args_invalid(build, walk, T, rows, w, n_pay, index, cap, sel_be32 != nullptr)) return fail(ctx, KZG_E_ARG, why);
    if (!ctx || !tab_be32 || !in_be32 || !out_slots || !out_home || !out_cnt || !out_missing || !out_first || !out_overrun ||
        (walk == 3 && !out_fetch_be32))
        return fail(ctx, KZG_E_ARG, "join: no context or no data");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    LaneHold H(ctx);
    if (int rc = H.take()) return rc;
    Lane& L = H.L();
    prof_begin(ctx, L);
    int rc = clear_flags(ctx, L);
    if (rc) return rc;
    hipStream_t s = L.stream;
    // the builders' layout: every column a vector of T canonical Montgomery elements, the table's w + n_pay first, then the w
    // columns of the one lookup or read, the selector, the fetched columns; slots, counters and homes in the staging buffer
    const uint64_t vw = T * 8;
    const uint32_t w_tab = w + n_pay, n_out = walk == 3 ? n_pay + (uint32_t)index : 0;
    HIPCHK(ctx, L.qext.ensure(((size_t)w_tab + w + 1 + n_out) * T * 32));
    HIPCHK(ctx, L.qstage.ensure(((size_t)cap + 3 * T) * 4));
    HIPCHK(ctx, L.scal.ensure(64));
    HIPCHK(ctx, L.out_be.ensure((size_t)(n_out ? n_out : 1) * T * 32));
    uint32_t *tab = L.qext.as<uint32_t>(), *in = tab + (uint64_t)w_tab * vw, *sel = in + (uint64_t)w * vw, *out = sel + vw;
    uint32_t *slots = L.qstage.as<uint32_t>(), *cnt = slots + cap, *home = cnt + T;
    uint64_t *missing = L.scal.as<uint64_t>(), *first = missing + 1;       // [0, 8) missing, [8, 16) first, [16, 20) overrun
    uint32_t* overrun = L.scal.as<uint32_t>() + 4;
    rc = upload_fr(ctx, L, tab_be32, (uint64_t)w_tab * T, tab, 1);
    if (rc) return rc;
    rc = upload_fr(ctx, L, in_be32, (uint64_t)w * T, in, 1);
    if (rc) return rc;
    if (walk == 2) {
        rc = upload_fr(ctx, L, sel_be32, T, sel, 1);
        if (rc) return rc;
    }
    HIPCHK(ctx, hipMemsetAsync(slots, 0xff, (size_t)cap * 4, s));
    HIPCHK(ctx, hipMemsetAsync(cnt, 0, (size_t)T * 4, s));
    HIPCHK(ctx, hipMemsetAsync(missing, 0, 64, s));
    HIPCHK(ctx, hipMemsetAsync(first, 0xff, 8, s));                        // KZG_FETCH_NONE
    // whatever the fetch fails to write must show: its columns start from a pattern that is no result
    if (n_out) HIPCHK(ctx, hipMemsetAsync(out, 0xff, (size_t)n_out * T * 32, s));
    launch_join_home(s, tab, T, w, T, cap, home);
    launch_join_home(s, in, T, w, T, cap, home + T);
    {
        Span sp(ctx, L, KZG_T_POLY);
        if (build == 0) launch_join_build(s, tab, T, w, slots, cap, overrun);
        else launch_join_build_rows(s, tab, T, rows, w, slots, cap, overrun);
        if (walk == 0) launch_join_probe(s, tab, in, T, w, slots, cap, cnt, missing, overrun);
        else if (walk == 1) launch_join_probe_rows(s, tab, in, T, rows, w, slots, cap, cnt, missing, overrun);
        else if (walk == 2) launch_join_probe_sel(s, tab, in, sel, T, rows, w, slots, cap, cnt, missing, overrun);
        else launch_join_fetch(s, tab, in, T, rows, w, n_pay, index != 0, slots, cap, out, missing, first, overrun);
    }
    // the fetched words as the kernel left them, taken out of Montgomery form without a reduction check (as kzg_test_recur_run)
    if (n_out) launch_fr_to_be(s, out, L.out_be.as<uint8_t>(), (uint64_t)n_out * T, 1);
    rc = finish(ctx, L);
    if (rc) return rc;
    HIPCHK(ctx, hipMemcpy(out_slots, slots, (size_t)cap * 4, hipMemcpyDeviceToHost));
    HIPCHK(ctx, hipMemcpy(out_cnt, cnt, (size_t)T * 4, hipMemcpyDeviceToHost));
    HIPCHK(ctx, hipMemcpy(out_home, home, (size_t)2 * T * 4, hipMemcpyDeviceToHost));
    if (n_out) HIPCHK(ctx, hipMemcpy(out_fetch_be32, L.out_be.p, (size_t)n_out * T * 32, hipMemcpyDeviceToHost));
    uint64_t tally[3];
    HIPCHK(ctx, hipMemcpy(tally, missing, sizeof tally, hipMemcpyDeviceToHost));
    *out_missing = tally[0];
    *out_first = tally[1];
    *out_overrun = (uint32_t)tally[2];
    H.clean = true;
    return KZG_OK;
}
int kzg_test_join_counts(kzg_ctx* ctx, const uint32_t* cnt, uint64_t n, uint8_t* out_be32) {
    if (!n || n > KZG_TEST_JOIN_MAX) return fail(ctx, KZG_E_ARG, "join counts: n outside [1, 2^12]");
    if (!ctx || !cnt || !out_be32) return fail(ctx, KZG_E_ARG, "join counts: no context or no data");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    LaneHold H(ctx);
    if (int rc = H.take()) return rc;
    Lane& L = H.L();
    prof_begin(ctx, L);
    int rc = clear_flags(ctx, L);
    if (rc) return rc;
    HIPCHK(ctx, L.qstage.ensure(n * 4));
    HIPCHK(ctx, L.coeffA.ensure(n * 32));
    HIPCHK(ctx, L.out_be.ensure(n * 32));
    HIPCHK(ctx, hipMemcpyAsync(L.qstage.p, cnt, n * 4, hipMemcpyHostToDevice, L.stream));
    launch_join_counts(L.stream, L.qstage.as<uint32_t>(), L.coeffA.as<uint32_t>(), n);
    launch_fr_to_be(L.stream, L.coeffA.as<uint32_t>(), L.out_be.as<uint8_t>(), n, 1);
    rc = finish(ctx, L);
    if (rc) return rc;
    HIPCHK(ctx, hipMemcpy(out_be32, L.out_be.p, n * 32, hipMemcpyDeviceToHost));
    H.clean = true;
    return KZG_OK;
}

// ---- the MSM passes of a multi-row call (tests/test_msm_passes_cpu.py)
int kzg_test_msm_passes(int c, int long_rows, uint32_t k, uint32_t m, uint32_t* out5, int* out_passes) {
    if (!out5 || !out_passes) return fail(nullptr, KZG_E_ARG, "msm passes: null output");
    if (c < 4 || c > 24 || k > KZG_MAX_BATCH_OPEN || m > KZG_MAX_OPEN_POINTS)
        return fail(nullptr, KZG_E_ARG, "msm passes: c in [4, 24], k <= 16 rows, m <= 4 tail sets");
    MsmPass pass[MR_SETS];
    *out_passes = (int)plan_msm_passes(c, 1u << (c - 1), long_rows != 0, k, m, pass);
    for (int p = 0; p < *out_passes; p++) {
        const uint32_t w[5] = {pass[p].row0, pass[p].nrows, pass[p].tail0, pass[p].ntail, pass[p].lane};
        memcpy(out5 + 5 * p, w, sizeof w);
    }
    return KZG_OK;
}

}  // extern "C"
