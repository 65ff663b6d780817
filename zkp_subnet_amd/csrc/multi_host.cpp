// multi_host.cpp -- kzg_multi_*: ONE handle for the G GPUs of a host (SURVEY 8b proposed kzg_create(device_count,
// device_ids); the reference builds one prover client per process: base/miner.py:73-84).  Written against the public C-ABI
// only; host threads only; nothing is exchanged between the devices but G x 192 bytes through the host.  Two layouts:
//   ROWS      worker index i is served by device i mod G, which holds exactly the slices of its workers -- the in-process
//             form of the reference's only distribution scheme (Pianist rows are independent, one row per miner: reference
//             neurons/validator.py:194-222).  No exchange at all.
//   SEGMENTS  one flat SRS cut into G contiguous segments, segment g on device g: ONE MSM runs as G partial MSMs, each on
//             its own device and lane, concurrently, and the G 192-byte partials are summed (BASELINE.json configs[3]; the
//             one-process form of what kzg_comm_* / kzg_msm_sharded do with one process per GPU).
// zkp_subnet_amd/multi.py is the same router one level up (with the text codec and the Client surface).
#include <string.h>

#include <algorithm>
#include <atomic>
#include <new>
#include <string>
#include <system_error>
#include <thread>
#include <vector>

#include "../../include/kzg_mi355x.h"

// The row-set calls do not go through the public kzg_rows_* exports but through the internal entries behind them (serve.hip),
// which take one argument more: expect_i, the slice every set named must belong to.  A handle of a set of ANOTHER worker
// on the same device is refused there; the public forms accept sets of any one worker.
#include "rows_impl.h"

namespace {
enum Layout { LAYOUT_NONE = 0, LAYOUT_ROWS_WHOLE, LAYOUT_ROWS_SLICED, LAYOUT_SEGMENTS };
struct SlotRange {      // what kzg_multi_upload_fr left on the devices: scalars of global points [offset, offset + n)
    uint64_t offset = 0, n = 0;
    bool valid = false;
};
}  // namespace

struct kzg_multi {
    std::vector<kzg_ctx*> ctx;
    std::vector<int> device;
    // ROWS_WHOLE: worker i = slice i of its device (every device holds the whole SRS); ROWS_SLICED: slice i / G (every device
    // holds only the slices it serves); SEGMENTS: device g holds global points [seg_lo[g], seg_lo[g] + seg_n[g]).
    // LAYOUT_NONE after ANY failed load: a load that failed on one device has already replaced the SRS on the others, so no
    // routing rule describes the devices any more -- every call is refused until a load succeeds on all of them.
    int layout = LAYOUT_NONE;
    int machines_scale = 0;
    uint64_t total_points = 0;
    std::vector<uint64_t> seg_lo, seg_n;
    SlotRange slot[4];
};

namespace {
thread_local std::string tl_multi_err;
int mfail(int code, const std::string& msg) {
    tl_multi_err = msg;
    return code;
}
// Joins whatever was started, whatever happens: an exception that unwound past joinable threads would be std::terminate --
// the miner process gone instead of a status code.
struct Joiner {
    std::vector<std::thread> th;
    ~Joiner() {
        for (auto& t : th)
            if (t.joinable()) t.join();
    }
};
// starts up to `want` threads running work(t); returns how many really started (allocation or thread-creation failures
// simply mean fewer helpers: the caller does the rest itself)
template <class F>
unsigned spawn(Joiner& j, unsigned want, F work) {
    unsigned started = 0;
    try {
        j.th.reserve(want);
        for (; started < want; started++) j.th.emplace_back(work, started);
    } catch (...) {
    }
    return started;
}
// runs fn(g) for every device on its own host thread (the per-GPU calls block); returns the first failure
template <class F>
int each_device(kzg_multi* m, F fn) {
    const int G = (int)m->ctx.size();
    std::vector<int> rc(G, KZG_OK);
    std::vector<std::string> msg(G);
    auto body = [&](int g) {
        rc[g] = fn(g);
        if (rc[g] != KZG_OK) msg[g] = kzg_last_error(m->ctx[g]);      // the message is per THREAD: fetch it on this one
    };
    {
        Joiner j;
        const unsigned started = spawn(j, (unsigned)(G - 1), [&](unsigned t) { body((int)t + 1); });
        body(0);
        for (int g = (int)started + 1; g < G; g++) body(g);          // no thread to be had: the caller does the rest
    }
    for (int g = 0; g < G; g++)
        if (rc[g] != KZG_OK) return mfail(rc[g], "device " + std::to_string(m->device[g]) + ": " + msg[g]);
    return KZG_OK;
}
int route(kzg_multi* m, uint32_t i, kzg_ctx** ctx, uint32_t* slice) {
    if (!m || m->ctx.empty()) return mfail(KZG_E_ARG, "no devices");
    if (m->layout == LAYOUT_SEGMENTS) return mfail(KZG_E_ARG, "the handle holds SRS segments (kzg_multi_msm), not worker rows");
    if (m->layout == LAYOUT_NONE) return mfail(KZG_E_ARG, "no SRS resident: call kzg_multi_load_srs_file / kzg_multi_gen_srs");
    if (i >= (1u << m->machines_scale)) return mfail(KZG_E_ARG, "worker index outside [0, 2^machines_scale)");
    const uint32_t G = (uint32_t)m->ctx.size();
    *ctx = m->ctx[i % G];
    *slice = m->layout == LAYOUT_ROWS_SLICED ? i / G : i;
    return KZG_OK;
}
int relay(kzg_ctx* ctx, int rc) {      // a per-GPU failure becomes this handle's last error (same thread)
    if (rc != KZG_OK) tl_multi_err = kzg_last_error(ctx);
    return rc;
}
// a call for worker i: routed to its device, run as call(ctx, slice), its failure relayed
template <class F>
int routed(kzg_multi* m, uint32_t i, F call) {
    kzg_ctx* c;
    uint32_t s;
    if (int rc = route(m, i, &c, &s)) return rc;
    return relay(c, call(c, s));
}
void forget(kzg_multi* m) {            // a load is about to replace the devices' SRS: nothing is routable until it has succeeded
    m->layout = LAYOUT_NONE;
    m->total_points = 0;
    for (auto& s : m->slot) s.valid = false;
}
// contiguous block partition of n points over G devices; sizes differ by at most one (zkp_subnet_amd.distributed.shard_range)
void shard_range(uint64_t n, uint64_t g, uint64_t G, uint64_t* lo, uint64_t* cnt) {
    const uint64_t base = n / G, extra = n % G;
    *lo = g * base + std::min(g, extra);
    *cnt = base + (g < extra ? 1 : 0);
}
int ceil_log2(uint64_t n) {
    int l = 0;
    while (((uint64_t)1 << l) < n) l++;
    return l;
}

int create_body(int device_count, const int* device_ids, kzg_multi** out) {
    if (!out) return KZG_E_ARG;
    *out = nullptr;
    if (device_count < 1 || device_count > 64 || !device_ids) return mfail(KZG_E_ARG, "1..64 devices");
    kzg_multi* m = new kzg_multi();
    struct Guard {                      // an exception below (vector growth) must not leak the contexts created so far
        kzg_multi* m;
        ~Guard() {
            if (!m) return;
            for (kzg_ctx* d : m->ctx) kzg_destroy(d);
            delete m;
        }
    } guard{m};
    m->ctx.reserve(device_count);
    m->device.reserve(device_count);
    m->seg_lo.assign(device_count, 0);
    m->seg_n.assign(device_count, 0);
    for (int k = 0; k < device_count; k++) {
        kzg_ctx* c = nullptr;
        const int rc = kzg_create(device_ids[k], &c);
        if (rc != KZG_OK) {
            const std::string why = kzg_last_error(nullptr);
            return mfail(rc, "device " + std::to_string(device_ids[k]) + ": " + why);
        }
        m->ctx.push_back(c);            // reserved: cannot throw
        m->device.push_back(device_ids[k]);
    }
    guard.m = nullptr;
    *out = m;
    return KZG_OK;
}

int load_srs_file_body(kzg_multi* m, const char* path, int compressed, int scale, int machines_scale) {
    if (!m || !path || machines_scale < 0 || machines_scale > 30) return mfail(KZG_E_ARG, "bad argument");
    const uint32_t G = (uint32_t)m->ctx.size();
    forget(m);
    // device g reads, checks and tabulates ONLY the slices of the worker indices it serves (i = g, g + G, ...): 1 / G of the
    // file, of the 34 GB of mainnet tables and of the start time each.  A device with no worker (G > slices) holds nothing.
    const int rc = each_device(m, [&](int g) {
        if ((uint64_t)g >= ((uint64_t)1 << machines_scale)) return (int)KZG_OK;
        return kzg_load_srs_file_slices(m->ctx[g], path, compressed, scale, machines_scale, (uint32_t)g, G);
    });
    if (rc != KZG_OK) return rc;        // the handle stays unloaded: some devices hold the new SRS, some the old one
    m->layout = LAYOUT_ROWS_SLICED;
    m->machines_scale = machines_scale;
    return KZG_OK;
}
int gen_srs_body(kzg_multi* m, const uint8_t tau_be32[32], const uint8_t* s0_be32_all, int scale, int machines_scale) {
    if (!m || !tau_be32 || !s0_be32_all || machines_scale < 0 || machines_scale > 20) return mfail(KZG_E_ARG, "bad argument");
    const uint32_t M = 1u << machines_scale, G = (uint32_t)m->ctx.size();
    forget(m);
    const int rc = each_device(m, [&](int g) {
        std::vector<uint8_t> mine;     // the factors of the worker indices this device serves, in slice order: i = g, g + G, ...
        for (uint32_t i = (uint32_t)g; i < M; i += G) mine.insert(mine.end(), s0_be32_all + 32 * (size_t)i, s0_be32_all + 32 * (size_t)i + 32);
        if (mine.empty()) return (int)KZG_OK;                          // more devices than rows: nothing to hold
        return kzg_gen_srs(m->ctx[g], tau_be32, mine.data(), (uint32_t)(mine.size() / 32), scale, machines_scale);
    });
    if (rc != KZG_OK) return rc;
    m->layout = LAYOUT_ROWS_SLICED;
    m->machines_scale = machines_scale;
    return KZG_OK;
}
void install_segments(kzg_multi* m, uint64_t n_points) {
    const uint64_t G = m->ctx.size();
    for (uint64_t g = 0; g < G; g++) shard_range(n_points, g, G, &m->seg_lo[g], &m->seg_n[g]);
    m->total_points = n_points;
    m->machines_scale = 0;
    m->layout = LAYOUT_SEGMENTS;
}
int load_segments_body(kzg_multi* m, const char* path, int compressed, uint64_t n_points) {
    if (!m || !path || !n_points) return mfail(KZG_E_ARG, "bad argument");
    const uint64_t G = m->ctx.size();
    if (n_points < G) return mfail(KZG_E_ARG, "fewer points than devices");
    forget(m);
    const int rc = each_device(m, [&](int g) {
        uint64_t lo, cnt;
        shard_range(n_points, (uint64_t)g, G, &lo, &cnt);
        return kzg_load_srs_file_range(m->ctx[g], path, compressed, lo, cnt, ceil_log2(cnt));
    });
    if (rc != KZG_OK) return rc;
    install_segments(m, n_points);
    return KZG_OK;
}
int gen_segments_body(kzg_multi* m, const uint8_t tau_be32[32], const uint8_t* s0_be32_per_device, uint64_t n_points) {
    if (!m || !tau_be32 || !s0_be32_per_device || !n_points) return mfail(KZG_E_ARG, "bad argument");
    const uint64_t G = m->ctx.size();
    if (n_points < G) return mfail(KZG_E_ARG, "fewer points than devices");
    forget(m);
    const int rc = each_device(m, [&](int g) {
        uint64_t lo, cnt;
        shard_range(n_points, (uint64_t)g, G, &lo, &cnt);
        // one slice of 2^ceil(log2 cnt) >= cnt points from the caller's factor tau^lo (the tail beyond cnt is never addressed)
        return kzg_gen_srs(m->ctx[g], tau_be32, s0_be32_per_device + 32 * (size_t)g, 1, ceil_log2(cnt), 0);
    });
    if (rc != KZG_OK) return rc;
    install_segments(m, n_points);
    return KZG_OK;
}
// the part of global points [offset, offset + n) that lives on device g: [*lo, *lo + *cnt), possibly empty
void overlap(const kzg_multi* m, int g, uint64_t offset, uint64_t n, uint64_t* lo, uint64_t* cnt) {
    const uint64_t a = std::max(offset, m->seg_lo[g]), b = std::min(offset + n, m->seg_lo[g] + m->seg_n[g]);
    *lo = a;
    *cnt = b > a ? b - a : 0;
}
int need_segments(kzg_multi* m, uint64_t offset, uint64_t n) {
    if (!m || m->ctx.empty()) return mfail(KZG_E_ARG, "no devices");
    if (m->layout != LAYOUT_SEGMENTS)
        return mfail(KZG_E_ARG, "no SRS segments resident: call kzg_multi_load_srs_file_segments / kzg_multi_gen_srs_segments");
    if (offset > m->total_points || n > m->total_points - offset) return mfail(KZG_E_ARG, "MSM range exceeds the resident SRS");
    return KZG_OK;
}
// G partial MSMs, each on its own device (and lane), concurrently; then ONE sum of the 192-byte partials.  `one(g, lo, cnt, out192)`
// computes device g's partial over global points [lo, lo + cnt).
template <class F>
int msm_over_segments(kzg_multi* m, uint64_t offset, uint64_t n, uint8_t out48[48], F one) {
    const int G = (int)m->ctx.size();
    std::vector<uint8_t> partials((size_t)G * 192);
    std::vector<int> used(G, 0);
    const int rc = each_device(m, [&](int g) {
        uint64_t lo, cnt;
        overlap(m, g, offset, n, &lo, &cnt);
        if (!cnt) return (int)KZG_OK;
        used[g] = 1;
        return one(g, lo, cnt, partials.data() + (size_t)192 * g);
    });
    if (rc != KZG_OK) return rc;
    uint32_t count = 0;
    for (int g = 0; g < G; g++)
        if (used[g]) {
            if ((int)count != g) memmove(partials.data() + (size_t)192 * count, partials.data() + (size_t)192 * g, 192);
            count++;
        }
    // G x 192 bytes through the host: no collective is worth building for that (a single-process RCCL communicator would add
    // a group launch over G streams to save one ~10-us copy); the sum runs on device 0's auxiliary stream
    return relay(m->ctx[0], kzg_g1_sum(m->ctx[0], partials.data(), count, out48));
}
int msm_body(kzg_multi* m, const uint8_t* scalars_be32, uint64_t n, uint64_t srs_offset, uint8_t out48[48]) {
    if (!out48 || (n && !scalars_be32)) return mfail(KZG_E_ARG, "bad argument");
    if (int rc = need_segments(m, srs_offset, n)) return rc;
    return msm_over_segments(m, srs_offset, n, out48, [&](int g, uint64_t lo, uint64_t cnt, uint8_t* out192) {
        return kzg_msm_partial(m->ctx[g], scalars_be32 + 32 * (size_t)(lo - srs_offset), cnt, lo - m->seg_lo[g], out192);
    });
}
int upload_body(kzg_multi* m, int slot, const uint8_t* scalars_be32, uint64_t n, uint64_t srs_offset) {
    if (slot < 0 || slot >= 4 || (n && !scalars_be32)) return mfail(KZG_E_ARG, "bad argument");
    if (int rc = need_segments(m, srs_offset, n)) return rc;
    m->slot[slot].valid = false;
    const int rc = each_device(m, [&](int g) {
        uint64_t lo, cnt;
        overlap(m, g, srs_offset, n, &lo, &cnt);
        return kzg_upload_fr(m->ctx[g], slot, cnt ? scalars_be32 + 32 * (size_t)(lo - srs_offset) : scalars_be32, cnt, 0);
    });
    if (rc != KZG_OK) return rc;
    m->slot[slot].offset = srs_offset;
    m->slot[slot].n = n;
    m->slot[slot].valid = true;
    return KZG_OK;
}
int msm_resident_body(kzg_multi* m, int slot, uint8_t out48[48]) {
    if (!m || slot < 0 || slot >= 4 || !out48) return mfail(KZG_E_ARG, "bad argument");
    if (!m->slot[slot].valid) return mfail(KZG_E_ARG, "the slot holds no scalars: kzg_multi_upload_fr first");
    const uint64_t offset = m->slot[slot].offset, n = m->slot[slot].n;
    if (int rc = need_segments(m, offset, n)) return rc;
    return msm_over_segments(m, offset, n, out48, [&](int g, uint64_t lo, uint64_t cnt, uint8_t* out192) {
        return kzg_msm_partial_resident(m->ctx[g], slot, cnt, lo - m->seg_lo[g], out192);
    });
}

// The rows of one challenge, all devices at once: row k (worker index indices[k], T x 32 bytes at rows_be32 + k * T * 32) runs
// on the device of its index, up to four rows per device in flight (a context has four lanes).  out_status[k] is that row's
// own status: one bad row never costs the others.  Returns KZG_OK when every row succeeded, else the first failing status.
int commit_open_rows_body(kzg_multi* m, uint32_t n_rows, const uint32_t* indices, const uint8_t* rows_be32, uint64_t T,
                          int evaluation_form, const uint8_t alpha_be32[32], uint8_t* out_c48, uint8_t* out_e32, uint8_t* out_p48,
                          int* out_status) {
    if (!m || (n_rows && (!indices || !rows_be32 || !alpha_be32 || !out_c48 || !out_e32 || !out_p48 || !out_status)))
        return mfail(KZG_E_ARG, "bad argument");
    if (!n_rows) return KZG_OK;
    std::atomic<uint32_t> next{0};
    std::vector<std::string> msg(n_rows);
    auto work = [&](unsigned) {
        for (uint32_t k; (k = next.fetch_add(1)) < n_rows;) {
            out_status[k] = kzg_multi_commit_open(m, indices[k], rows_be32 + (size_t)k * T * 32, T, evaluation_form, alpha_be32,
                                                  out_c48 + 48 * (size_t)k, out_e32 + 32 * (size_t)k, out_p48 + 48 * (size_t)k);
            if (out_status[k] != KZG_OK) msg[k] = tl_multi_err;
        }
    };
    {
        Joiner j;
        const unsigned want = (unsigned)std::min<size_t>(n_rows, 4 * m->ctx.size());
        (void)spawn(j, want - 1, work);
        work(0);                       // (rows are claimed from one counter: fewer helpers only means fewer rows in flight)
    }
    for (uint32_t k = 0; k < n_rows; k++)
        if (out_status[k] != KZG_OK) return mfail(out_status[k], "row " + std::to_string(k) + " (worker " + std::to_string(indices[k]) + "): " + msg[k]);
    return KZG_OK;
}

// the entry points that allocate (vectors, strings, threads): no exception crosses the C boundary
template <class F>
int guarded(const char* who, F f) {
    try {
        return f();
    } catch (const std::bad_alloc&) {
        return mfail(KZG_E_NOMEM, std::string(who) + ": out of host memory");
    } catch (...) {
        return mfail(KZG_E_HIP, std::string(who) + ": unexpected host-side failure");
    }
}
}  // namespace

extern "C" {

void kzg_multi_destroy(kzg_multi* m) {
    if (!m) return;
    for (kzg_ctx* c : m->ctx) kzg_destroy(c);
    delete m;
}
const char* kzg_multi_last_error(kzg_multi*) { return tl_multi_err.c_str(); }
int kzg_multi_count(kzg_multi* m) { return m ? (int)m->ctx.size() : 0; }
kzg_ctx* kzg_multi_ctx(kzg_multi* m, int k) { return (m && k >= 0 && k < (int)m->ctx.size()) ? m->ctx[k] : nullptr; }
int kzg_multi_device_of(kzg_multi* m, uint32_t i) { return (m && !m->ctx.empty()) ? m->device[i % m->ctx.size()] : -1; }

int kzg_multi_commit(kzg_multi* m, uint32_t i, const uint8_t* row_be32, uint64_t T, int evaluation_form, uint8_t out48[48]) {
    return routed(m, i, [&](kzg_ctx* c, uint32_t s) { return kzg_commit(c, s, row_be32, T, evaluation_form, out48); });
}
int kzg_multi_open(kzg_multi* m, uint32_t i, const uint8_t* row_be32, uint64_t T, int evaluation_form, const uint8_t alpha_be32[32],
                   uint8_t out_eval32[32], uint8_t out_proof48[48]) {
    return routed(m, i, [&](kzg_ctx* c, uint32_t s) {
        return kzg_open(c, s, row_be32, T, evaluation_form, alpha_be32, out_eval32, out_proof48);
    });
}
int kzg_multi_commit_open(kzg_multi* m, uint32_t i, const uint8_t* row_be32, uint64_t T, int evaluation_form,
                          const uint8_t alpha_be32[32], uint8_t out48[48], uint8_t out_eval32[32], uint8_t out_proof48[48]) {
    return routed(m, i, [&](kzg_ctx* c, uint32_t s) {
        return kzg_commit_open(c, s, row_be32, T, evaluation_form, alpha_be32, out48, out_eval32, out_proof48);
    });
}
int kzg_multi_commit_open_batch(kzg_multi* m, uint32_t i, uint32_t k, const uint8_t* rows_be32, uint64_t T, int evaluation_form,
                                const uint8_t alpha_be32[32], const uint8_t gamma_be32[32], uint8_t* out_commitments48,
                                uint8_t* out_evals32, uint8_t out_proof48[48]) {
    return routed(m, i, [&](kzg_ctx* c, uint32_t s) {
        return kzg_commit_open_batch(c, s, k, rows_be32, T, evaluation_form, alpha_be32, gamma_be32, out_commitments48, out_evals32,
                                     out_proof48);
    });
}
int kzg_multi_commit_open_multi(kzg_multi* mh, uint32_t i, uint32_t k, const uint8_t* rows_be32, uint64_t T,
                                int evaluation_form, uint32_t m, const uint8_t* points_be32, const uint32_t* masks,
                                const uint8_t* gammas_be32, uint8_t* out_commitments48, uint8_t* out_evals32,
                                uint8_t* out_proofs48) {
    return routed(mh, i, [&](kzg_ctx* c, uint32_t s) {
        return kzg_commit_open_multi(c, s, k, rows_be32, T, evaluation_form, m, points_be32, masks, gammas_be32, out_commitments48,
                                     out_evals32, out_proofs48);
    });
}
int kzg_multi_rows_commit(kzg_multi* mh, uint32_t i, uint32_t k, const uint8_t* rows_be32, uint64_t T, int evaluation_form,
                          uint8_t* out_commitments48, uint64_t* out_handle) {
    return routed(mh, i, [&](kzg_ctx* c, uint32_t s) {
        return kzg_rows_commit(c, s, k, rows_be32, T, evaluation_form, out_commitments48, out_handle);
    });
}
int kzg_multi_rows_commit_typed(kzg_multi* mh, uint32_t i, uint32_t k, const kzg_col* cols, uint64_t T, int evaluation_form,
                                uint8_t* out_commitments48, uint64_t* out_handle) {
    return routed(mh, i, [&](kzg_ctx* c, uint32_t s) {
        return kzg_rows_commit_typed(c, s, k, cols, T, evaluation_form, out_commitments48, out_handle);
    });
}
// from here on every call is the entry its single-context twin (serve.hip) calls, with the slice as expect_i
int kzg_multi_rows_read(kzg_multi* mh, uint32_t i, uint32_t n_handles, const uint64_t* handles, uint32_t row, uint64_t first,
                        uint64_t count, uint32_t kind, int evaluation_form, void* out, uint64_t out_overflow[2]) {
    return routed(mh, i, [&](kzg_ctx* c, uint32_t s) {
        return kzg_impl::rows_read(c, s, n_handles, handles, row, first, count, kind, evaluation_form, out, out_overflow);
    });
}
int kzg_multi_rows_open(kzg_multi* mh, uint32_t i, uint32_t n_handles, const uint64_t* handles, uint32_t m,
                        const uint8_t* points_be32, const uint32_t* masks, const uint8_t* gammas_be32, uint8_t* out_evals32,
                        uint8_t* out_proofs48) {
    return routed(mh, i, [&](kzg_ctx* c, uint32_t s) {
        return kzg_impl::rows_open(c, s, n_handles, handles, m, points_be32, masks, gammas_be32, out_evals32, out_proofs48);
    });
}
int kzg_multi_rows_eval(kzg_multi* mh, uint32_t i, uint32_t n_handles, const uint64_t* handles, uint32_t m,
                        const uint8_t* points_be32, const uint32_t* masks, uint8_t* out_evals32) {
    return routed(mh, i, [&](kzg_ctx* c, uint32_t s) {
        return kzg_impl::rows_eval(c, s, n_handles, handles, m, points_be32, masks, out_evals32);
    });
}
int kzg_multi_rows_open_lincomb(kzg_multi* mh, uint32_t i, uint32_t n_handles, const uint64_t* handles, uint32_t k,
                                uint32_t m, const uint8_t* points_be32, const uint8_t* coeffs_be32, uint8_t* out_values32,
                                uint8_t* out_proofs48) {
    return routed(mh, i, [&](kzg_ctx* c, uint32_t s) {
        return kzg_impl::rows_lincomb(c, s, n_handles, handles, k, m, points_be32, coeffs_be32, out_values32, out_proofs48);
    });
}
int kzg_multi_rows_commit_shplonk(kzg_multi* mh, uint32_t i, uint32_t n_handles, const uint64_t* handles, uint32_t k, uint32_t m,
                                  const uint8_t* points_be32, const uint32_t* masks, const uint8_t* coeffs_be32,
                                  uint8_t out_commitment48[48], uint64_t* out_handle) {
    return routed(mh, i, [&](kzg_ctx* c, uint32_t s) {
        return kzg_impl::rows_shplonk(c, s, n_handles, handles, k, m, points_be32, masks, coeffs_be32, out_commitment48,
                                      out_handle);
    });
}
int kzg_multi_rows_commit_grand_product(kzg_multi* mh, uint32_t i, uint32_t n_wire_handles, const uint64_t* wire_handles,
                                        uint32_t n_sigma_handles, const uint64_t* sigma_handles, uint32_t k,
                                        const uint8_t* shifts_be32, const uint8_t beta_be32[32], const uint8_t gamma_be32[32],
                                        uint8_t out_commitment48[48], uint8_t out_closing32[32], uint64_t* out_handle) {
    return routed(mh, i, [&](kzg_ctx* c, uint32_t s) {
        return kzg_impl::rows_grand_product(c, s, n_wire_handles, wire_handles, n_sigma_handles, sigma_handles, k, shifts_be32,
                                            beta_be32, gamma_be32, out_commitment48, out_closing32, out_handle, nullptr, nullptr);
    });
}
int kzg_multi_rows_commit_grand_product_zk(kzg_multi* mh, uint32_t i, uint32_t n_wire_handles, const uint64_t* wire_handles,
                                           uint32_t n_sigma_handles, const uint64_t* sigma_handles, uint32_t k,
                                           const uint8_t* shifts_be32, const uint8_t beta_be32[32], const uint8_t gamma_be32[32],
                                           uint64_t usable, const uint8_t* tail_be32, uint8_t out_commitment48[48],
                                           uint8_t out_closing32[32], uint64_t* out_handle) {
    const kzg_impl::Blind zk = {usable, tail_be32};
    return routed(mh, i, [&](kzg_ctx* c, uint32_t s) {
        return kzg_impl::rows_grand_product(c, s, n_wire_handles, wire_handles, n_sigma_handles, sigma_handles, k, shifts_be32,
                                            beta_be32, gamma_be32, out_commitment48, out_closing32, out_handle, &zk, nullptr);
    });
}
int kzg_multi_rows_commit_grand_product_chain(kzg_multi* mh, uint32_t i, uint32_t n_wire_handles, const uint64_t* wire_handles,
                                              uint32_t n_sigma_handles, const uint64_t* sigma_handles, uint32_t k,
                                              const uint8_t* shifts_be32, const uint8_t beta_be32[32],
                                              const uint8_t gamma_be32[32], uint64_t usable, const uint8_t* tail_be32,
                                              const uint8_t start_be32[32], uint8_t out_commitment48[48],
                                              uint8_t out_closing32[32], uint64_t* out_handle) {
    const kzg_impl::Blind zk = {usable, tail_be32};
    return routed(mh, i, [&](kzg_ctx* c, uint32_t s) {
        if (!start_be32) return (int)KZG_E_ARG;   // (to the entry a null start means "not a chain")
        return kzg_impl::rows_grand_product(c, s, n_wire_handles, wire_handles, n_sigma_handles, sigma_handles, k, shifts_be32,
                                            beta_be32, gamma_be32, out_commitment48, out_closing32, out_handle, &zk, start_be32);
    });
}
int kzg_multi_rows_commit_shuffle(kzg_multi* mh, uint32_t i, uint32_t n_input_handles, const uint64_t* input_handles,
                                  uint32_t n_shuffle_handles, const uint64_t* shuffle_handles, uint32_t n_groups, uint32_t width,
                                  const uint8_t theta_be32[32], const uint8_t gamma_be32[32], const kzg_shuffle_opts* opts,
                                  uint8_t out_commitment48[48], uint8_t out_closing32[32], uint64_t* out_handle) {
    return routed(mh, i, [&](kzg_ctx* c, uint32_t s) {
        return kzg_impl::rows_shuffle(c, s, n_input_handles, input_handles, n_shuffle_handles, shuffle_handles, n_groups, width,
                                      theta_be32, gamma_be32, opts, out_commitment48, out_closing32, out_handle);
    });
}
int kzg_multi_rows_commit_sorted(kzg_multi* mh, uint32_t i, uint32_t n_input_handles, const uint64_t* input_handles, uint32_t width,
                                 uint32_t n_keys, const kzg_sorted_opts* opts, uint8_t* out_commitments48, uint64_t* out_handle) {
    return routed(mh, i, [&](kzg_ctx* c, uint32_t s) {
        return kzg_impl::rows_sorted(c, s, n_input_handles, input_handles, width, n_keys, opts, out_commitments48, out_handle);
    });
}
int kzg_multi_rows_commit_sigma(kzg_multi* mh, uint32_t i, uint32_t n_label_handles, const uint64_t* label_handles, uint32_t k,
                                const uint8_t* shifts_be32, const kzg_sigma_opts* opts, uint8_t* out_commitments48,
                                uint64_t out_stats[2], uint64_t* out_handle) {
    return routed(mh, i, [&](kzg_ctx* c, uint32_t s) {
        return kzg_impl::rows_sigma(c, s, n_label_handles, label_handles, k, shifts_be32, opts, out_commitments48, out_stats,
                                    out_handle);
    });
}
int kzg_multi_rows_check_copies(kzg_multi* mh, uint32_t i, uint32_t n_wire_handles, const uint64_t* wire_handles,
                                uint32_t n_label_handles, const uint64_t* label_handles, uint32_t k, const kzg_sigma_opts* opts,
                                uint64_t out[2]) {
    return routed(mh, i, [&](kzg_ctx* c, uint32_t s) {
        return kzg_impl::rows_check_copies(c, s, n_wire_handles, wire_handles, n_label_handles, label_handles, k, opts, out);
    });
}
int kzg_multi_rows_commit_derived(kzg_multi* mh, uint32_t i, uint32_t n_input_handles, const uint64_t* input_handles,
                                  uint32_t n_ops, const kzg_derive_op* ops, const kzg_derive_opts* opts,
                                  uint8_t* out_commitments48, uint64_t* out_counts, uint64_t* out_handle) {
    return routed(mh, i, [&](kzg_ctx* c, uint32_t s) {
        return kzg_impl::rows_derived(c, s, n_input_handles, input_handles, n_ops, ops, opts, out_commitments48, out_counts,
                                      out_handle);
    });
}
int kzg_multi_rows_commit_int(kzg_multi* mh, uint32_t i, uint32_t n_input_handles, const uint64_t* input_handles, uint32_t n_ops,
                              const kzg_int_op* ops, const kzg_derive_opts* opts, uint8_t* out_commitments48,
                              uint64_t* out_counts, uint64_t* out_first, uint64_t* out_handle) {
    return routed(mh, i, [&](kzg_ctx* c, uint32_t s) {
        return kzg_impl::rows_int(c, s, n_input_handles, input_handles, n_ops, ops, opts, out_commitments48, out_counts,
                                  out_first, out_handle);
    });
}
int kzg_multi_rows_commit_alu(kzg_multi* mh, uint32_t i, uint32_t n_input_handles, const uint64_t* input_handles,
                              uint32_t n_entries, const kzg_alu_entry* program, uint32_t n_units, const kzg_alu_unit* units,
                              const kzg_derive_opts* opts, uint8_t* out_commitments48, uint64_t* out_counts, uint64_t* out_first,
                              uint64_t* out_unknown, uint64_t* out_first_unknown, uint64_t* out_handle) {
    return routed(mh, i, [&](kzg_ctx* c, uint32_t s) {
        return kzg_impl::rows_alu(c, s, n_input_handles, input_handles, n_entries, program, n_units, units, opts,
                                  out_commitments48, out_counts, out_first, out_unknown, out_first_unknown, out_handle);
    });
}
int kzg_multi_rows_commit_wide(kzg_multi* mh, uint32_t i, uint32_t n_input_handles, const uint64_t* input_handles, uint32_t n_ops,
                               const kzg_wide_op* ops, const kzg_derive_opts* opts, uint8_t* out_commitments48,
                               uint64_t* out_counts, uint64_t* out_first, uint64_t* out_qover, uint64_t* out_first_qover,
                               uint64_t* out_handle) {
    return routed(mh, i, [&](kzg_ctx* c, uint32_t s) {
        return kzg_impl::rows_wide(c, s, n_input_handles, input_handles, n_ops, ops, opts, out_commitments48, out_counts,
                                   out_first, out_qover, out_first_qover, out_handle);
    });
}
int kzg_multi_rows_commit_poseidon(kzg_multi* mh, uint32_t i, uint32_t n_input_handles, const uint64_t* input_handles,
                                   const kzg_poseidon_params* params, uint32_t n_units, const kzg_poseidon_unit* units,
                                   const kzg_derive_opts* opts, uint8_t* out_commitments48, uint64_t* out_perms,
                                   uint64_t* out_mismatch, uint64_t* out_first_mismatch, uint64_t* out_handle) {
    return routed(mh, i, [&](kzg_ctx* c, uint32_t s) {
        return kzg_impl::rows_poseidon(c, s, n_input_handles, input_handles, params, n_units, units, opts, out_commitments48,
                                       out_perms, out_mismatch, out_first_mismatch, out_handle);
    });
}
int kzg_multi_rows_commit_poseidon2(kzg_multi* mh, uint32_t i, uint32_t n_input_handles, const uint64_t* input_handles,
                                    const kzg_poseidon2_params* params, uint32_t n_units, const kzg_poseidon_unit* units,
                                    const kzg_derive_opts* opts, uint8_t* out_commitments48, uint64_t* out_perms,
                                    uint64_t* out_mismatch, uint64_t* out_first_mismatch, uint64_t* out_handle) {
    return routed(mh, i, [&](kzg_ctx* c, uint32_t s) {
        return kzg_impl::rows_poseidon2(c, s, n_input_handles, input_handles, params, n_units, units, opts, out_commitments48,
                                        out_perms, out_mismatch, out_first_mismatch, out_handle);
    });
}
int kzg_multi_rows_commit_poseidon_chain(kzg_multi* mh, uint32_t i, uint32_t n_input_handles, const uint64_t* input_handles,
                                         const kzg_poseidon_params* params, uint32_t n_units,
                                         const kzg_poseidon_chain_unit* units, const kzg_derive_opts* opts,
                                         uint8_t* out_commitments48, uint64_t* out_blocks, uint64_t* out_segments,
                                         uint64_t* out_bad_pos, uint64_t* out_first_bad_pos, uint64_t* out_mismatch,
                                         uint64_t* out_first_mismatch, uint64_t* out_handle) {
    uint64_t* const st[6] = {out_blocks, out_segments, out_bad_pos, out_first_bad_pos, out_mismatch, out_first_mismatch};
    return routed(mh, i, [&](kzg_ctx* c, uint32_t s) {
        return kzg_impl::rows_poseidon_chain(c, s, n_input_handles, input_handles, params, n_units, units, opts, out_commitments48,
                                             st, out_handle);
    });
}
int kzg_multi_rows_commit_sha256(kzg_multi* mh, uint32_t i, uint32_t n_input_handles, const uint64_t* input_handles,
                                 uint32_t n_units, const kzg_sha256_unit* units, const kzg_derive_opts* opts,
                                 uint8_t* out_commitments48, uint64_t* out_blocks, uint64_t* out_messages, uint64_t* out_counts,
                                 uint64_t* out_first, uint64_t* out_mismatch, uint64_t* out_first_mismatch, uint64_t* out_handle) {
    return routed(mh, i, [&](kzg_ctx* c, uint32_t s) {
        return kzg_impl::rows_sha256(c, s, n_input_handles, input_handles, n_units, units, opts, out_commitments48, out_blocks,
                                     out_messages, out_counts, out_first, out_mismatch, out_first_mismatch, out_handle);
    });
}
int kzg_multi_rows_commit_keccak(kzg_multi* mh, uint32_t i, uint32_t n_input_handles, const uint64_t* input_handles,
                                 uint32_t n_units, const kzg_keccak_unit* units, const kzg_derive_opts* opts,
                                 uint8_t* out_commitments48, uint64_t* out_perms, uint64_t* out_messages, uint64_t* out_counts,
                                 uint64_t* out_first, uint64_t* out_mismatch, uint64_t* out_first_mismatch, uint64_t* out_handle) {
    return routed(mh, i, [&](kzg_ctx* c, uint32_t s) {
        return kzg_impl::rows_keccak(c, s, n_input_handles, input_handles, n_units, units, opts, out_commitments48, out_perms,
                                     out_messages, out_counts, out_first, out_mismatch, out_first_mismatch, out_handle);
    });
}
int kzg_multi_rows_commit_ec(kzg_multi* mh, uint32_t i, uint32_t n_input_handles, const uint64_t* input_handles,
                             const kzg_ec_curve* curve, uint32_t n_units, const kzg_ec_unit* units, const kzg_derive_opts* opts,
                             uint8_t* out_commitments48, uint64_t* out_counts, uint64_t* out_first, uint64_t* out_singular,
                             uint64_t* out_first_singular, uint64_t* out_mismatch, uint64_t* out_first_mismatch,
                             uint64_t* out_unknown, uint64_t* out_first_unknown, uint64_t* out_segments, uint64_t* out_handle) {
    uint64_t* const st[9] = {out_counts,         out_first,   out_singular,      out_first_singular, out_mismatch,
                             out_first_mismatch, out_unknown, out_first_unknown, out_segments};
    return routed(mh, i, [&](kzg_ctx* c, uint32_t s) {
        return kzg_impl::rows_ec(c, s, n_input_handles, input_handles, curve, n_units, units, opts, out_commitments48, st,
                                 out_handle);
    });
}
int kzg_multi_rows_commit_edwards(kzg_multi* mh, uint32_t i, uint32_t n_input_handles, const uint64_t* input_handles,
                                  const kzg_edwards_curve* curve, uint32_t n_units, const kzg_edwards_unit* units,
                                  const kzg_derive_opts* opts, uint8_t* out_commitments48, uint64_t* out_singular,
                                  uint64_t* out_first_singular, uint64_t* out_mismatch, uint64_t* out_first_mismatch,
                                  uint64_t* out_unknown, uint64_t* out_first_unknown, uint64_t* out_segments,
                                  uint64_t* out_handle) {
    uint64_t* const st[7] = {out_singular, out_first_singular, out_mismatch, out_first_mismatch,
                             out_unknown,  out_first_unknown,  out_segments};
    return routed(mh, i, [&](kzg_ctx* c, uint32_t s) {
        return kzg_impl::rows_edwards(c, s, n_input_handles, input_handles, curve, n_units, units, opts, out_commitments48, st,
                                      out_handle);
    });
}
int kzg_multi_rows_commit_expr(kzg_multi* mh, uint32_t i, uint32_t n_input_handles, const uint64_t* input_handles,
                               uint32_t n_exprs, const kzg_expr* exprs, const kzg_expr_opts* opts, uint8_t* out_commitments48,
                               uint64_t* out_nonzero, uint64_t* out_first, uint64_t* out_handle) {
    return routed(mh, i, [&](kzg_ctx* c, uint32_t s) {
        return kzg_impl::rows_expr(c, s, n_input_handles, input_handles, n_exprs, exprs, opts, out_commitments48, out_nonzero,
                                   out_first, out_handle);
    });
}
int kzg_multi_rows_commit_recurrence(kzg_multi* mh, uint32_t i, uint32_t n_input_handles, const uint64_t* input_handles,
                                     uint32_t n_recs, const kzg_recurrence* recs, const kzg_recurrence_opts* opts,
                                     uint8_t* out_commitments48, uint8_t* out_closings32, uint64_t* out_handle) {
    return routed(mh, i, [&](kzg_ctx* c, uint32_t s) {
        return kzg_impl::rows_recurrence(c, s, n_input_handles, input_handles, n_recs, recs, opts, out_commitments48,
                                         out_closings32, out_handle);
    });
}
int kzg_multi_rows_commit_fetch(kzg_multi* mh, uint32_t i, uint32_t n_input_handles, const uint64_t* input_handles,
                                uint32_t n_table_handles, const uint64_t* table_handles, uint32_t n_reads, uint32_t n_keys,
                                uint32_t flags, const kzg_derive_opts* opts, uint8_t* out_commitments48, uint64_t* out_missing,
                                uint64_t* out_first_missing, uint64_t* out_handle) {
    return routed(mh, i, [&](kzg_ctx* c, uint32_t s) {
        return kzg_impl::rows_fetch(c, s, n_input_handles, input_handles, n_table_handles, table_handles, n_reads, n_keys, flags,
                                    opts, out_commitments48, out_missing, out_first_missing, out_handle);
    });
}
int kzg_multi_rows_commit_lookup_sum(kzg_multi* mh, uint32_t i, uint32_t n_input_handles, const uint64_t* input_handles,
                                     uint32_t n_table_handles, const uint64_t* table_handles, uint64_t mult_handle,
                                     uint32_t n_lookups, uint32_t width, const uint8_t theta_be32[32],
                                     const uint8_t beta_be32[32], uint8_t out_commitment48[48], uint8_t out_closing32[32],
                                     uint64_t* out_handle) {
    return routed(mh, i, [&](kzg_ctx* c, uint32_t s) {
        return kzg_impl::rows_lookup_sum(c, s, n_input_handles, input_handles, n_table_handles, table_handles, mult_handle,
                                         n_lookups, width, theta_be32, beta_be32, out_commitment48, out_closing32, out_handle,
                                         nullptr, nullptr);
    });
}
int kzg_multi_rows_commit_lookup_sum_zk(kzg_multi* mh, uint32_t i, uint32_t n_input_handles, const uint64_t* input_handles,
                                        uint32_t n_table_handles, const uint64_t* table_handles, uint64_t mult_handle,
                                        uint32_t n_lookups, uint32_t width, const uint8_t theta_be32[32],
                                        const uint8_t beta_be32[32], uint64_t usable, const uint8_t* tail_be32,
                                        uint8_t out_commitment48[48], uint8_t out_closing32[32], uint64_t* out_handle) {
    const kzg_impl::Blind zk = {usable, tail_be32};
    return routed(mh, i, [&](kzg_ctx* c, uint32_t s) {
        return kzg_impl::rows_lookup_sum(c, s, n_input_handles, input_handles, n_table_handles, table_handles, mult_handle,
                                         n_lookups, width, theta_be32, beta_be32, out_commitment48, out_closing32, out_handle,
                                         &zk, nullptr);
    });
}
int kzg_multi_rows_commit_lookup_sum_sel(kzg_multi* mh, uint32_t i, uint32_t n_input_handles, const uint64_t* input_handles,
                                         uint32_t n_table_handles, const uint64_t* table_handles, uint64_t mult_handle,
                                         uint32_t n_sel_handles, const uint64_t* sel_handles, const uint32_t* sel_index,
                                         uint32_t n_lookups, uint32_t width, const uint8_t theta_be32[32],
                                         const uint8_t beta_be32[32], uint64_t usable, const uint8_t* tail_be32,
                                         uint8_t out_commitment48[48], uint8_t out_closing32[32], uint64_t* out_handle) {
    const kzg_impl::Blind zk = {usable, tail_be32};
    const kzg_impl::SelCall sc = {n_sel_handles, sel_handles, sel_index};
    return routed(mh, i, [&](kzg_ctx* c, uint32_t s) {
        return kzg_impl::rows_lookup_sum(c, s, n_input_handles, input_handles, n_table_handles, table_handles, mult_handle,
                                         n_lookups, width, theta_be32, beta_be32, out_commitment48, out_closing32, out_handle,
                                         &zk, &sc);
    });
}
int kzg_multi_rows_commit_multiplicities(kzg_multi* mh, uint32_t i, uint32_t n_input_handles, const uint64_t* input_handles,
                                         uint32_t n_table_handles, const uint64_t* table_handles, uint32_t n_lookups,
                                         uint32_t width, uint8_t out_commitment48[48], uint64_t* out_missing,
                                         uint64_t* out_handle) {
    return routed(mh, i, [&](kzg_ctx* c, uint32_t s) {
        return kzg_impl::rows_multiplicities(c, s, n_input_handles, input_handles, n_table_handles, table_handles, n_lookups,
                                             width, out_commitment48, out_missing, out_handle, nullptr, nullptr);
    });
}
int kzg_multi_rows_commit_multiplicities_zk(kzg_multi* mh, uint32_t i, uint32_t n_input_handles, const uint64_t* input_handles,
                                            uint32_t n_table_handles, const uint64_t* table_handles, uint32_t n_lookups,
                                            uint32_t width, uint64_t usable, const uint8_t* tail_be32,
                                            uint8_t out_commitment48[48], uint64_t* out_missing, uint64_t* out_handle) {
    const kzg_impl::Blind zk = {usable, tail_be32};
    return routed(mh, i, [&](kzg_ctx* c, uint32_t s) {
        return kzg_impl::rows_multiplicities(c, s, n_input_handles, input_handles, n_table_handles, table_handles, n_lookups,
                                             width, out_commitment48, out_missing, out_handle, &zk, nullptr);
    });
}
int kzg_multi_rows_commit_multiplicities_sel(kzg_multi* mh, uint32_t i, uint32_t n_input_handles, const uint64_t* input_handles,
                                             uint32_t n_table_handles, const uint64_t* table_handles, uint32_t n_sel_handles,
                                             const uint64_t* sel_handles, const uint32_t* sel_index, uint32_t n_lookups,
                                             uint32_t width, uint64_t usable, const uint8_t* tail_be32,
                                             uint8_t out_commitment48[48], uint64_t* out_missing, uint64_t* out_handle) {
    const kzg_impl::Blind zk = {usable, tail_be32};
    const kzg_impl::SelCall sc = {n_sel_handles, sel_handles, sel_index};
    return routed(mh, i, [&](kzg_ctx* c, uint32_t s) {
        return kzg_impl::rows_multiplicities(c, s, n_input_handles, input_handles, n_table_handles, table_handles, n_lookups,
                                             width, out_commitment48, out_missing, out_handle, &zk, &sc);
    });
}
int kzg_multi_rows_commit_quotient(kzg_multi* mh, uint32_t i, uint32_t n_handles, const uint64_t* handles,
                                   const kzg_quotient_gate* gate, const kzg_quotient_perm* perm, uint32_t ext_log,
                                   uint32_t n_pieces, uint8_t* out_commitments48, uint64_t* out_handle) {
    return routed(mh, i, [&](kzg_ctx* c, uint32_t s) {
        if (!gate) return (int)KZG_E_ARG;
        const kzg_quotient_terms terms = kzg_impl::quotient_plain_terms(gate);
        return kzg_impl::rows_quotient(c, s, n_handles, handles, &terms, perm, nullptr, nullptr, nullptr, ext_log, n_pieces,
                                       out_commitments48, out_handle, true);
    });
}
int kzg_multi_rows_commit_quotient_ext(kzg_multi* mh, uint32_t i, uint32_t n_handles, const uint64_t* handles,
                                       const kzg_quotient_terms* gate, const kzg_quotient_perm* perm,
                                       const kzg_quotient_lookup* lookup, uint32_t ext_log, uint32_t n_pieces,
                                       uint8_t* out_commitments48, uint64_t* out_handle) {
    return routed(mh, i, [&](kzg_ctx* c, uint32_t s) {
        return kzg_impl::rows_quotient(c, s, n_handles, handles, gate, perm, lookup, nullptr, nullptr, ext_log, n_pieces,
                                       out_commitments48, out_handle, false);
    });
}
int kzg_multi_rows_commit_quotient_zk(kzg_multi* mh, uint32_t i, uint32_t n_handles, const uint64_t* handles,
                                      const kzg_quotient_terms* gate, const kzg_quotient_perm* perm,
                                      const kzg_quotient_lookup* lookup, const kzg_quotient_active* active, uint32_t ext_log,
                                      uint32_t n_pieces, uint8_t* out_commitments48, uint64_t* out_handle) {
    return routed(mh, i, [&](kzg_ctx* c, uint32_t s) {
        return kzg_impl::rows_quotient(c, s, n_handles, handles, gate, perm, lookup, nullptr, active, ext_log, n_pieces,
                                       out_commitments48, out_handle, false);
    });
}
int kzg_multi_rows_commit_quotient_sel(kzg_multi* mh, uint32_t i, uint32_t n_handles, const uint64_t* handles,
                                       const kzg_quotient_terms* gate, const kzg_quotient_perm* perm,
                                       const kzg_quotient_lookup* lookup, const kzg_quotient_selectors* selectors,
                                       const kzg_quotient_active* active, uint32_t ext_log, uint32_t n_pieces,
                                       uint8_t* out_commitments48, uint64_t* out_handle) {
    return routed(mh, i, [&](kzg_ctx* c, uint32_t s) {
        return kzg_impl::rows_quotient(c, s, n_handles, handles, gate, perm, lookup, selectors, active, ext_log, n_pieces,
                                       out_commitments48, out_handle, false);
    });
}
int kzg_multi_rows_quotient_part(kzg_multi* mh, uint32_t i, uint32_t n_handles, const uint64_t* handles,
                                 const kzg_quotient_terms* gate, const kzg_quotient_perm* perm, const kzg_quotient_link* link,
                                 const kzg_quotient_lookup* lookup, const kzg_quotient_active* active, uint32_t ext_log,
                                 const uint8_t* scale_be32, uint64_t* inout_acc) {
    return routed(mh, i, [&](kzg_ctx* c, uint32_t s) {
        return kzg_impl::rows_quotient_part(c, s, n_handles, handles, gate, perm, link, lookup, nullptr, active, ext_log,
                                            scale_be32, inout_acc);
    });
}
int kzg_multi_rows_quotient_part_sel(kzg_multi* mh, uint32_t i, uint32_t n_handles, const uint64_t* handles,
                                     const kzg_quotient_terms* gate, const kzg_quotient_perm* perm, const kzg_quotient_link* link,
                                     const kzg_quotient_lookup* lookup, const kzg_quotient_selectors* selectors,
                                     const kzg_quotient_active* active, uint32_t ext_log, const uint8_t* scale_be32,
                                     uint64_t* inout_acc) {
    return routed(mh, i, [&](kzg_ctx* c, uint32_t s) {
        return kzg_impl::rows_quotient_part(c, s, n_handles, handles, gate, perm, link, lookup, selectors, active, ext_log,
                                            scale_be32, inout_acc);
    });
}
int kzg_multi_rows_quotient_finish(kzg_multi* mh, uint32_t i, uint64_t acc, uint32_t n_pieces, uint8_t* out_commitments48,
                                   uint64_t* out_handle) {
    return routed(mh, i, [&](kzg_ctx* c, uint32_t s) {
        return kzg_impl::rows_quotient_finish(c, s, acc, n_pieces, out_commitments48, out_handle);
    });
}
int kzg_multi_rows_release(kzg_multi* mh, uint32_t i, uint64_t handle) {
    return routed(mh, i, [&](kzg_ctx* c, uint32_t s) { return kzg_impl::rows_release(c, s, handle); });
}

int kzg_multi_create(int device_count, const int* device_ids, kzg_multi** out) {
    return guarded("kzg_multi_create", [&] { return create_body(device_count, device_ids, out); });
}
int kzg_multi_load_srs_file(kzg_multi* m, const char* path, int compressed, int scale, int machines_scale) {
    return guarded("kzg_multi_load_srs_file", [&] { return load_srs_file_body(m, path, compressed, scale, machines_scale); });
}
int kzg_multi_gen_srs(kzg_multi* m, const uint8_t tau_be32[32], const uint8_t* s0_be32_all, int scale, int machines_scale) {
    return guarded("kzg_multi_gen_srs", [&] { return gen_srs_body(m, tau_be32, s0_be32_all, scale, machines_scale); });
}
int kzg_multi_load_srs_file_segments(kzg_multi* m, const char* path, int compressed, uint64_t n_points) {
    return guarded("kzg_multi_load_srs_file_segments", [&] { return load_segments_body(m, path, compressed, n_points); });
}
int kzg_multi_gen_srs_segments(kzg_multi* m, const uint8_t tau_be32[32], const uint8_t* s0_be32_per_device, uint64_t n_points) {
    return guarded("kzg_multi_gen_srs_segments", [&] { return gen_segments_body(m, tau_be32, s0_be32_per_device, n_points); });
}
int kzg_multi_segment(kzg_multi* m, int g, uint64_t out_first_count[2]) {
    if (!m || !out_first_count || g < 0 || g >= (int)m->ctx.size() || m->layout != LAYOUT_SEGMENTS) return mfail(KZG_E_ARG, "no such segment");
    out_first_count[0] = m->seg_lo[g];
    out_first_count[1] = m->seg_n[g];
    return KZG_OK;
}
int kzg_multi_msm(kzg_multi* m, const uint8_t* scalars_be32, uint64_t n, uint64_t srs_offset, uint8_t out48[48]) {
    return guarded("kzg_multi_msm", [&] { return msm_body(m, scalars_be32, n, srs_offset, out48); });
}
int kzg_multi_upload_fr(kzg_multi* m, int slot, const uint8_t* scalars_be32, uint64_t n, uint64_t srs_offset) {
    return guarded("kzg_multi_upload_fr", [&] { return upload_body(m, slot, scalars_be32, n, srs_offset); });
}
int kzg_multi_msm_resident(kzg_multi* m, int slot, uint8_t out48[48]) {
    return guarded("kzg_multi_msm_resident", [&] { return msm_resident_body(m, slot, out48); });
}
int kzg_multi_commit_open_rows(kzg_multi* m, uint32_t n_rows, const uint32_t* indices, const uint8_t* rows_be32, uint64_t T,
                               int evaluation_form, const uint8_t alpha_be32[32], uint8_t* out_c48, uint8_t* out_e32, uint8_t* out_p48,
                               int* out_status) {
    return guarded("kzg_multi_commit_open_rows", [&] {
        return commit_open_rows_body(m, n_rows, indices, rows_be32, T, evaluation_form, alpha_be32, out_c48, out_e32, out_p48, out_status);
    });
}

}  // extern "C"
