// C-ABI of libdemethify_hip.so, part 1: the context -- errors, the per-family HIP-event timers, the memory pool that every
// device buffer of the library comes from, and the upload staging of the restart loops.
#include "dmf_api.h"
#include "dmf_mt_jump.h"

namespace dmf_api {

static thread_local char g_last_error[512] = "";

int hip_fail(hipError_t e, const char* what, const char* file, int line) {
    snprintf(g_last_error, sizeof(g_last_error), "%s failed at %s:%d: %s", what, file, line, hipGetErrorString(e));
    return DMF_ERR_HIP;
}

int clock_drain(dmf_context* ctx, FamilyClock& c) {
    if (c.used == 0) return DMF_OK;
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    for (int i = 0; i < c.used; ++i) {
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, c.start[i], c.stop[i]));
        c.total_ms += ms;
    }
    c.launches += c.used;
    c.used = 0;
    return DMF_OK;
}

// Device buffers come from a stream-ordered memory pool OF THE CONTEXT'S OWN on the context's stream.  The pool keeps
// what is freed (release threshold raised in dmf_context_create; the device's default pool, which other users of a
// borrowed device share, is left alone), so the multi-GB buffers of a problem or a solver that is destroyed and
// re-created with the same sizes -- every bootstrap replicate does that -- are handed back without a trip to the
// driver (hipMalloc / hipFree of 2 GB cost tens of milliseconds each).
static bool pool_enabled() {  // DEMETHIFY_NO_POOL=1: plain hipMalloc / hipFree (debugging aid)
    static const bool on = [] {
        const char* v = getenv("DEMETHIFY_NO_POOL");
        return !(v != nullptr && v[0] == '1');
    }();
    return on;
}
// Above the pool: freed blocks of 1 MB and more are kept by exact size and handed to the next allocation of that size
// (a bootstrap replicate frees and re-allocates the same seven multi-GB buffers; hipFreeAsync + hipMallocFromPoolAsync
// cost ~0.2 ms per large block even when the pool keeps the memory).  Everything that touches these blocks is enqueued
// on the context's one stream, so a block can be reused the moment it is "freed".  At most kKeepPerSize blocks per size
// and kKeepBytes in total are kept; the rest goes back to the pool.
constexpr size_t kKeepMinBytes = (size_t)1 << 20, kKeepBytes = (size_t)24 << 30;
constexpr int kKeepPerSize = 3;
hipError_t pool_alloc(dmf_context* ctx, void** p, size_t bytes) {
    if (!pool_enabled() || ctx->pool == nullptr) return hipMalloc(p, bytes);
    if (bytes >= kKeepMinBytes) {
        auto it = ctx->kept.find(bytes);
        if (it != ctx->kept.end() && !it->second.empty()) {
            *p = it->second.back();
            it->second.pop_back();
            ctx->kept_bytes -= bytes;
            ctx->live[*p] = bytes;
            return hipSuccess;
        }
    }
    hipError_t e = hipMallocFromPoolAsync(p, bytes, ctx->pool, ctx->stream);
    if (e != hipSuccess && ctx->kept_bytes > 0) {  // out of memory with blocks parked here: give them back, try again
        (void)hipGetLastError();
        for (auto& kv : ctx->kept)
            for (void* q : kv.second) (void)hipFreeAsync(q, ctx->stream);
        ctx->kept.clear();
        ctx->kept_bytes = 0;
        (void)hipStreamSynchronize(ctx->stream);
        e = hipMallocFromPoolAsync(p, bytes, ctx->pool, ctx->stream);
    }
    if (e == hipSuccess && bytes >= kKeepMinBytes) ctx->live[*p] = bytes;
    return e;
}
void pool_free(dmf_context* ctx, void* p) {
    if (p == nullptr) return;
    if (!pool_enabled() || ctx->pool == nullptr) {
        (void)hipStreamSynchronize(ctx->stream);
        (void)hipFree(p);
        return;
    }
    auto it = ctx->live.find(p);
    if (it != ctx->live.end()) {
        const size_t bytes = it->second;
        ctx->live.erase(it);
        auto& slot = ctx->kept[bytes];
        if ((int)slot.size() < kKeepPerSize && ctx->kept_bytes + bytes <= kKeepBytes) {
            slot.push_back(p);
            ctx->kept_bytes += bytes;
            return;
        }
    }
    (void)hipFreeAsync(p, ctx->stream);
}

// A block for the staging calls: from the pool on the given stream, past the kept lists (which belong to the thread that
// drives `stream`; dmf_stage_upload and dmf_mask_draw run on worker threads), and its release before anybody else has seen
// the block.
hipError_t stage_alloc(dmf_context* ctx, hipStream_t st, void** p, size_t bytes) {
    if (!pool_enabled() || ctx->pool == nullptr) return hipMalloc(p, bytes);
    return hipMallocFromPoolAsync(p, bytes, ctx->pool, st);
}
void stage_release(dmf_context* ctx, hipStream_t st, void* p) {
    if (!pool_enabled() || ctx->pool == nullptr) (void)hipFree(p);
    else (void)hipFreeAsync(p, st);
}

int export_array(dmf_context* ctx, const void* dev_src, size_t bytes, int flags, void* dst) {
    if (bytes == 0 || dst == nullptr) return DMF_OK;
    const hipMemcpyKind kind = (flags & DMF_PTR_DEVICE) ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    HIP_TRY(hipMemcpyAsync(dst, dev_src, bytes, kind, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return DMF_OK;
}

int check_ctx(dmf_context* ctx) {
    if (ctx == nullptr) return DMF_ERR_BAD_ARG;
    HIP_TRY(hipSetDevice(ctx->device));
    return DMF_OK;
}

// The keys of W >= 2 segments of c blocks, made on the device from row 0 of keys[W][624], the caller's key (block 0): row
// s >= 1 is the key of block c s - 1 (see k_mask_draw_segments).  By rounds of radix R = kJumpRadix, one launch each with a
// workgroup per key and no workgroup waiting for another: the first makes rows 1..min(R, W - 1) from row 0 (jumps of c s - 1
// blocks); then, with rows [1, d] at hand, a round makes rows src + k d (k = 1..R - 1, src in [1, d]) by jumps of c d k blocks
// and multiplies d by R -- ceil(log_R (W - 1)) launches (two for 1024 segments) on at most 2 R - 1 polynomials.  The job
// table and the term lists of the last (c, W) stay on the device.  Under copy_mutex, on the copy stream.
constexpr int64_t kJumpRadix = 32;
int mask_jump_keys(dmf_context* ctx, unsigned int* keys, int64_t c, int64_t W, hipStream_t st) {
    if (ctx->mask_jump_table == nullptr || ctx->mask_jump_c != c || ctx->mask_jump_w != W) {
        std::vector<unsigned short> terms;
        std::vector<dmf::MtJumpJob> jobs;
        std::vector<std::pair<size_t, size_t>> rounds;
        std::unordered_map<uint64_t, std::pair<int, int>> placed;  // blocks -> { first, n_terms } in `terms`
        auto add = [&](int64_t src, int64_t dst, uint64_t blocks) {
            auto it = placed.find(blocks);
            if (it == placed.end()) {
                const std::vector<uint16_t>& t = dmf::mt_jump_terms(blocks);
                it = placed.emplace(blocks, std::make_pair((int)terms.size(), (int)t.size())).first;
                terms.insert(terms.end(), t.begin(), t.end());
            }
            jobs.push_back({(int)src, (int)dst, it->second.first, it->second.second});
        };
        int64_t d = kJumpRadix < W - 1 ? kJumpRadix : W - 1;
        for (int64_t s = 1; s <= d; ++s) add(0, s, (uint64_t)c * (uint64_t)s - 1);
        rounds.push_back({0, jobs.size()});
        while (d < W - 1) {
            const size_t first = jobs.size();
            for (int64_t k = 1; k < kJumpRadix && k * d + 1 <= W - 1; ++k)
                for (int64_t src = 1; src <= d && src + k * d <= W - 1; ++src)
                    add(src, src + k * d, (uint64_t)c * (uint64_t)d * (uint64_t)k);
            rounds.push_back({first, jobs.size() - first});
            d = kJumpRadix * d < W - 1 ? kJumpRadix * d : W - 1;
        }
        if (ctx->mask_jump_table != nullptr) (void)hipFree(ctx->mask_jump_table);  // (no draw is in flight: each waits for its own)
        ctx->mask_jump_table = nullptr;
        const size_t job_bytes = jobs.size() * sizeof(dmf::MtJumpJob), term_bytes = terms.size() * sizeof(unsigned short);
        char* table = nullptr;
        HIP_TRY(hipMalloc((void**)&table, job_bytes + term_bytes));
        hipError_t e = hipMemcpyAsync(table, jobs.data(), job_bytes, hipMemcpyHostToDevice, st);
        e = e != hipSuccess ? e : hipMemcpyAsync(table + job_bytes, terms.data(), term_bytes, hipMemcpyHostToDevice, st);
        e = e != hipSuccess ? e : hipStreamSynchronize(st);
        if (e != hipSuccess) {
            (void)hipFree(table);
            return hip_fail(e, "mask_jump_keys", __FILE_NAME__, __LINE__);
        }
        ctx->mask_jump_table = table, ctx->mask_jump_terms_at = job_bytes, ctx->mask_jump_c = c, ctx->mask_jump_w = W;
        ctx->mask_jump_rounds = std::move(rounds);
    }
    const dmf::MtJumpJob* jobs = reinterpret_cast<const dmf::MtJumpJob*>(ctx->mask_jump_table);
    const unsigned short* terms = reinterpret_cast<const unsigned short*>(ctx->mask_jump_table + ctx->mask_jump_terms_at);
    for (const auto& round : ctx->mask_jump_rounds)
        HIP_TRY(dmf::launch_mt_jump(keys, jobs + round.first, (int64_t)round.second, terms, st));
    return DMF_OK;
}

static_assert(dmf::kMaskDrawMaxSegments == DMF_MASK_DRAW_MAX_SEGMENTS, "the header's constant is the kernels'");

// dmf_mask_draw and dmf_mask_draw_segments.  blocks_per_segment: 0 the plan's choice, -1 one workgroup, >= 1 as given.
int mask_draw(dmf_context* ctx, uint32_t key[624], int* pos, int64_t N, int64_t S, uint64_t threshold,
              int64_t blocks_per_segment, void** out_bits, int64_t* n_kept) {
    if (ctx == nullptr || key == nullptr || pos == nullptr || out_bits == nullptr || n_kept == nullptr) return DMF_ERR_BAD_ARG;
    *out_bits = nullptr;
    if (*pos < 0 || *pos > 624 || N < 1 || S < 1 || threshold > ((uint64_t)1 << 53) || blocks_per_segment < -1)
        return DMF_ERR_BAD_ARG;
    if (S > dmf::kMaskDrawMaxS || N > dmf::kMaskDrawMaxElements / S) return DMF_ERR_UNSUPPORTED;
    int64_t c = blocks_per_segment;  // below: -1 = the one-workgroup kernel
    if (c == 0) {
        int64_t segments = 0;
        dmf::mask_draw_plan(N, S, &segments, &c);
        if (segments == 1) c = -1;
    } else if (c >= 1 && (dmf::mask_draw_blocks(N, S) + c - 1) / c > dmf::kMaskDrawMaxSegments) {
        return DMF_ERR_BAD_ARG;
    }
    // the segments in use, W: up to the block of the last word, which the position moves by at most one; keys are made for
    // all the W_keys >= W segments of the shape, so that the folds of a sweep share one set of polynomials
    const int64_t W = c < 1 ? 1 : (int64_t)(((uint64_t)*pos + 2 * (uint64_t)N * (uint64_t)S - 1) / 624 / (uint64_t)c) + 1;
    const int64_t W_keys = c < 1 ? 1 : (dmf::mask_draw_blocks(N, S) + c - 1) / c;
    HIP_TRY(hipSetDevice(ctx->device));  // (the current device is per thread)
    std::lock_guard<std::mutex> lock(ctx->copy_mutex);
    if (ctx->copy_stream == nullptr) HIP_TRY(hipStreamCreateWithFlags(&ctx->copy_stream, hipStreamNonBlocking));
    const hipStream_t st = ctx->copy_stream;
    // the key, then { ones, position } as two u64 (8-byte aligned: 624 is even), then the ones per segment
    const size_t state_words = 624 + 4 + (c < 1 ? 0 : 2 * (size_t)W_keys);
    DevBuf<unsigned char> bits;
    DevBuf<uint32_t> state, keys;
    HIP_TRY(bits.alloc_staged(ctx, (size_t)N * (size_t)((S + 7) / 8), st));
    HIP_TRY(state.alloc_staged(ctx, state_words, st));
    std::vector<uint32_t> h_state(state_words, 0);
    unsigned long long* d_result = reinterpret_cast<unsigned long long*>(state + 624);
    if (c < 1) {
        std::memcpy(h_state.data(), key, 624 * sizeof(uint32_t));
        HIP_TRY(hipMemcpyAsync(state, h_state.data(), (624 + 4) * sizeof(uint32_t), hipMemcpyHostToDevice, st));
        HIP_TRY(dmf::launch_mask_draw(state, *pos, N, S, threshold, bits, d_result, st));
    } else {
        HIP_TRY(keys.alloc_staged(ctx, 624 * (size_t)W_keys, st));
        HIP_TRY(hipMemcpyAsync(keys, key, 624 * sizeof(uint32_t), hipMemcpyHostToDevice, st));
        if (W_keys >= 2) DMF_TRY(mask_jump_keys(ctx, keys, c, W_keys, st));
        HIP_TRY(dmf::launch_mask_draw_segments(keys, state, *pos, c, N, S, threshold, bits, d_result, d_result + 2, st));
    }
    HIP_TRY(hipMemcpyAsync(h_state.data(), state, state_words * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    std::vector<unsigned long long> result((state_words - 624) / 2);
    std::memcpy(result.data(), h_state.data() + 624, result.size() * sizeof(unsigned long long));
    unsigned long long ones = result[0];
    if (c >= 1) {
        ones = 0;
        for (int64_t s = 0; s < W; ++s) ones += result[2 + (size_t)s];  // (integers, segment by segment)
    }
    std::memcpy(key, h_state.data(), 624 * sizeof(uint32_t));
    *pos = (int)result[1];
    *n_kept = (int64_t)ones;
    *out_bits = bits.release();
    return DMF_OK;
}

}  // namespace dmf_api

using namespace dmf_api;

extern "C" {

const char* dmf_status_string(int status) {
    switch (status) {
        case DMF_OK: return "ok";
        case DMF_ERR_BAD_ARG: return "bad argument";
        case DMF_ERR_BAD_SHAPE: return "shape mismatch";
        case DMF_ERR_HIP: return "HIP runtime error";
        case DMF_ERR_NONFINITE: return "non-finite input";
        case DMF_ERR_UNSUPPORTED: return "unsupported size";
        case DMF_ERR_NO_DEVICE: return "no gfx950 device";
        default: return "unknown status";
    }
}

const char* dmf_last_error(void) { return g_last_error; }

int dmf_abi_version(void) { return 1; }

int dmf_context_create(int device, void* stream, dmf_context** out) {
    if (out == nullptr) return DMF_ERR_BAD_ARG;
    *out = nullptr;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return DMF_ERR_NO_DEVICE;
    if (device < 0 || device >= count) return DMF_ERR_BAD_ARG;
    HIP_TRY(hipSetDevice(device));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        snprintf(g_last_error, sizeof(g_last_error), "device %d is %s, this library is built for gfx950",
                 device, prop.gcnArchName);
        return DMF_ERR_NO_DEVICE;
    }
    dmf_context* ctx = new (std::nothrow) dmf_context();
    if (ctx == nullptr) return DMF_ERR_BAD_ARG;
    ctx->device = device;
    if (stream != nullptr) {
        ctx->stream = (hipStream_t)stream;
    } else {
        hipError_t e = hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking);
        if (e != hipSuccess) {
            delete ctx;
            return hip_fail(e, "hipStreamCreate", __FILE_NAME__, __LINE__);
        }
        ctx->own_stream = true;
    }
    hipError_t e = hipMalloc((void**)&ctx->scratch, 4096 * sizeof(double));
    if (e != hipSuccess) {
        if (ctx->own_stream) hipStreamDestroy(ctx->stream);
        delete ctx;
        return hip_fail(e, "hipMalloc(scratch)", __FILE_NAME__, __LINE__);
    }
    // a pool of the context's own that keeps freed memory for the next problem / solver of the same size (see
    // pool_alloc); if the runtime cannot create one, plain hipMalloc / hipFree are used
    if (pool_enabled()) {
        hipMemPoolProps props = {};
        props.allocType = hipMemAllocationTypePinned;
        props.handleTypes = hipMemHandleTypeNone;
        props.location.type = hipMemLocationTypeDevice;
        props.location.id = device;
        if (hipMemPoolCreate(&ctx->pool, &props) == hipSuccess && ctx->pool != nullptr) {
            uint64_t keep = UINT64_MAX;
            (void)hipMemPoolSetAttribute(ctx->pool, hipMemPoolAttrReleaseThreshold, &keep);
        } else {
            ctx->pool = nullptr;
            (void)hipGetLastError();
        }
    }
    *out = ctx;
    return DMF_OK;
}

int dmf_context_destroy(dmf_context* ctx) {
    if (ctx == nullptr) return DMF_OK;
    hipSetDevice(ctx->device);
    hipStreamSynchronize(ctx->stream);
    for (auto& c : ctx->clocks) {
        for (auto ev : c.start) hipEventDestroy(ev);
        for (auto ev : c.stop) hipEventDestroy(ev);
    }
    hipFree(ctx->scratch);
    for (auto& kv : ctx->kept)
        for (void* q : kv.second) (void)hipFreeAsync(q, ctx->stream);
    ctx->kept.clear();
    (void)hipStreamSynchronize(ctx->stream);
    for (void* h : ctx->pinned_states) (void)hipHostFree(h);
    for (double* h : ctx->pinned_moms) (void)hipHostFree(h);
    for (hipEvent_t ev : ctx->events) (void)hipEventDestroy(ev);
    if (ctx->copy_stream != nullptr) {
        hipStreamSynchronize(ctx->copy_stream);
        hipStreamDestroy(ctx->copy_stream);
    }
    if (ctx->mask_jump_table != nullptr) (void)hipFree(ctx->mask_jump_table);
    if (ctx->pool != nullptr) (void)hipMemPoolDestroy(ctx->pool);  // hands the cached buffers back to the driver
    if (ctx->own_stream) hipStreamDestroy(ctx->stream);
    delete ctx;
    return DMF_OK;
}

/* Staging for a restart loop (demethify/demethify.py:165-171,195-201): the next restart's initialisation goes to the
 * device from a worker thread, on a copy stream of the context's own, while `stream` runs the current restart; the
 * solver is then created from the device copy (DMF_PTR_DEVICE).  Thread-safe; returns when the copy is complete. */
int dmf_stage_upload(dmf_context* ctx, const void* host, size_t bytes, void** out_dev) {
    if (ctx == nullptr || host == nullptr || out_dev == nullptr || bytes == 0) return DMF_ERR_BAD_ARG;
    HIP_TRY(hipSetDevice(ctx->device));  // (the current device is per thread)
    std::lock_guard<std::mutex> lock(ctx->copy_mutex);
    if (ctx->copy_stream == nullptr) HIP_TRY(hipStreamCreateWithFlags(&ctx->copy_stream, hipStreamNonBlocking));
    void* d = nullptr;
    HIP_TRY(stage_alloc(ctx, ctx->copy_stream, &d, bytes));
    hipError_t e = hipMemcpyAsync(d, host, bytes, hipMemcpyHostToDevice, ctx->copy_stream);
    e = e != hipSuccess ? e : hipStreamSynchronize(ctx->copy_stream);
    if (e != hipSuccess) {
        stage_release(ctx, ctx->copy_stream, d);
        return hip_fail(e, "dmf_stage_upload", __FILE_NAME__, __LINE__);
    }
    *out_dev = d;
    return DMF_OK;
}

int dmf_stage_download(dmf_context* ctx, const void* dev, size_t bytes, void* host) {
    if (ctx == nullptr || dev == nullptr || host == nullptr || bytes == 0) return DMF_ERR_BAD_ARG;
    HIP_TRY(hipSetDevice(ctx->device));
    std::lock_guard<std::mutex> lock(ctx->copy_mutex);
    if (ctx->copy_stream == nullptr) HIP_TRY(hipStreamCreateWithFlags(&ctx->copy_stream, hipStreamNonBlocking));
    HIP_TRY(hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, ctx->copy_stream));
    HIP_TRY(hipStreamSynchronize(ctx->copy_stream));
    return DMF_OK;
}

/* The hold-out mask of a bi-cross-validation fold (ic.py:68, `np.random.rand(*meth_f.shape) < fraction`) drawn where it
 * is used: numpy's MT19937 stream is continued on the copy stream (dmf_kernels_rng.hip), under dmf_stage_upload's threading
 * contract -- by one persistent workgroup where the plan says one segment, else by one workgroup per segment, on keys that
 * jump-ahead rounds make from the caller's.  No kernel-family clock: a FamilyScope records on `stream`, which another thread
 * drives. */
int dmf_mask_draw(dmf_context* ctx, uint32_t key[624], int* pos, int64_t N, int64_t S, uint64_t threshold, void** out_bits,
                  int64_t* n_kept) {
    return mask_draw(ctx, key, pos, N, S, threshold, 0, out_bits, n_kept);
}

int dmf_mask_draw_segments(dmf_context* ctx, uint32_t key[624], int* pos, int64_t N, int64_t S, uint64_t threshold,
                           int64_t blocks_per_segment, void** out_bits, int64_t* n_kept) {
    return mask_draw(ctx, key, pos, N, S, threshold, blocks_per_segment, out_bits, n_kept);
}

int dmf_mask_draw_plan(int64_t N, int64_t S, int64_t* segments, int64_t* blocks_per_segment) {
    if (segments == nullptr || blocks_per_segment == nullptr || N < 1 || S < 1) return DMF_ERR_BAD_ARG;
    if (S > dmf::kMaskDrawMaxS || N > dmf::kMaskDrawMaxElements / S) return DMF_ERR_UNSUPPORTED;
    dmf::mask_draw_plan(N, S, segments, blocks_per_segment);
    return DMF_OK;
}

int dmf_stage_free(dmf_context* ctx, void* dev) {
    if (ctx == nullptr) return DMF_ERR_BAD_ARG;
    if (dev == nullptr) return DMF_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    pool_free(ctx, dev);  // ordered behind the work of `stream` that read it
    return DMF_OK;
}

int dmf_context_synchronize(dmf_context* ctx) {
    DMF_TRY(check_ctx(ctx));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return DMF_OK;
}

int dmf_context_set_profiling(dmf_context* ctx, int enabled) {
    DMF_TRY(check_ctx(ctx));
    if (!enabled)
        for (auto& c : ctx->clocks) DMF_TRY(clock_drain(ctx, c));
    // 0 = off, 1 = every family, otherwise a mask with bit (1 + family) set for the families to time
    // (2 = DMF_KERNEL_ROWPASS only, ...): each timed launch costs two event records on the stream
    ctx->profiling = enabled == 0 ? 0u : enabled == 1 ? ~0u : (unsigned)enabled >> 1;
    return DMF_OK;
}

int dmf_context_kernel_time(dmf_context* ctx, int family, double* total_ms, int64_t* launches) {
    DMF_TRY(check_ctx(ctx));
    if (family < 0 || family >= DMF_KERNEL_FAMILIES) return DMF_ERR_BAD_ARG;
    FamilyClock& c = ctx->clocks[family];
    DMF_TRY(clock_drain(ctx, c));
    if (total_ms) *total_ms = c.total_ms;
    if (launches) *launches = c.launches;
    return DMF_OK;
}

int dmf_context_reset_kernel_time(dmf_context* ctx) {
    DMF_TRY(check_ctx(ctx));
    for (auto& c : ctx->clocks) {
        DMF_TRY(clock_drain(ctx, c));
        c.total_ms = 0.0;
        c.launches = 0;
    }
    return DMF_OK;
}

int dmf_context_set_generic(dmf_context* ctx, int enabled) {
    if (ctx == nullptr) return DMF_ERR_BAD_ARG;
    if (enabled < 0 || enabled > 4) return DMF_ERR_BAD_ARG;
    ctx->generic_level = enabled;
    return DMF_OK;
}

int dmf_context_set_x16(dmf_context* ctx, int enabled) {
    if (ctx == nullptr || enabled < 0 || enabled > 1) return DMF_ERR_BAD_ARG;
    ctx->x16 = enabled != 0;
    return DMF_OK;
}

int dmf_context_set_rowpass_pair(dmf_context* ctx, int enabled) {
    if (ctx == nullptr || enabled < 0 || enabled > 1) return DMF_ERR_BAD_ARG;
    ctx->rowpass_pair = enabled != 0;
    return DMF_OK;
}

int dmf_context_set_rowpass_defer_c(dmf_context* ctx, int enabled) {
    if (ctx == nullptr || enabled < 0 || enabled > 1) return DMF_ERR_BAD_ARG;
    ctx->rowpass_defer_c = enabled != 0;
    return DMF_OK;
}

int dmf_context_set_rowpass_bytes(dmf_context* ctx, int enabled) {
    if (ctx == nullptr || enabled < 0 || enabled > 1) return DMF_ERR_BAD_ARG;
    ctx->rowpass_bytes = enabled != 0;
    return DMF_OK;
}

int dmf_context_set_stop_confirmation(dmf_context* ctx, int mode) {
    if (ctx == nullptr || mode < 0 || mode > 2) return DMF_ERR_BAD_ARG;
    ctx->stop_confirmation = mode;
    return DMF_OK;
}

}  // extern "C"
