// dm2_api.hip -- extern "C" entry points of libdm2_hip.so (include/dm2_hip.h).
// Host orchestration equivalent to CudaRenderer::Renderer::forward/backward and
// RenderLayerGenerator::forward (renderer.cu:78-269, 271-392, 509-674), without
// the reference's per-stage cudaDeviceSynchronize (auxiliary.h:433-440): the
// only host wait is the read-back of the pair count in the plan step.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
#include <string>

#include "dm2_device_math.h"
#include "dm2_stamps.h"
#include "dm2_state.h"

#ifdef DM2_STAMPS
namespace dm2 {
unsigned long long* stamps_table() {
    static unsigned long long* p = nullptr;
    if (!p) { (void)hipMalloc((void**)&p, 2 * DM2_NSTAMP * sizeof(unsigned long long)); (void)hipMemset(p, 0, 2 * DM2_NSTAMP * sizeof(unsigned long long)); }
    return p;
}
}  // namespace dm2
#endif

namespace {

thread_local std::string g_err;

int fail(const std::string& m) { g_err = m; return 1; }

#define DM2_HIP(expr)                                                                         \
    do {                                                                                      \
        hipError_t e_ = (expr);                                                               \
        if (e_ != hipSuccess) return fail(std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

struct PinnedWord {     // per-thread mapped host words for the plan's read-back
    uint32_t* p = nullptr;      // host view: [0] num_rendered [1] longest tile list [2,3] pair bound [4] sequence word
    uint32_t* dp = nullptr;     // device view of the same memory, for device `dev`
    int dev = -1;
    uint32_t seq = 0;
    hipEvent_t ev = nullptr;
    ~PinnedWord() { if (p) (void)hipHostFree(p); if (ev) (void)hipEventDestroy(ev); }
};
thread_local PinnedWord g_pin;

// (num_rendered, entries of the longest tile list) of a plan: the one host read-back of a forward.  The plan's last kernel
// stores them into mapped host memory and then a sequence word; the host polls that word (microseconds instead of the
// ~30 us of a copy command + event).  Should the word not show up in time (a platform that delays such stores until the
// kernel has retired), the classical route takes over: an event behind a device-to-host copy of the device-side words.
int plan_meta_prepare(uint32_t** host_meta_dev, uint32_t* seq) {
    if (!g_pin.p) {
        DM2_HIP(hipHostMalloc((void**)&g_pin.p, 64, hipHostMallocMapped | hipHostMallocPortable));
        for (int k = 0; k < 8; k++) g_pin.p[k] = 0u;
    }
    int cur = 0;
    DM2_HIP(hipGetDevice(&cur));
    if (cur != g_pin.dev) {                                               // (a thread that moves to another GPU: that GPU's view)
        void* dp = nullptr;
        DM2_HIP(hipHostGetDevicePointer(&dp, g_pin.p, 0));
        g_pin.dp = (uint32_t*)dp; g_pin.dev = cur;
        if (g_pin.ev) { (void)hipEventDestroy(g_pin.ev); g_pin.ev = nullptr; }     // (events belong to a device as well)
    }
    if (!g_pin.ev) DM2_HIP(hipEventCreateWithFlags(&g_pin.ev, hipEventDisableTiming));
    g_pin.seq = g_pin.seq + 1u ? g_pin.seq + 1u : 1u;                      // never 0: the words start out as 0
    *host_meta_dev = g_pin.dp; *seq = g_pin.seq;
    return 0;
}
int plan_meta_wait(const uint32_t* plan_meta, hipStream_t st, int64_t* num_rendered, int64_t* max_tile_entries, int64_t* pair_bound) {
    DM2_HIP(hipEventRecord(g_pin.ev, st));                                 // (also tells whether the plan has retired)
    volatile uint32_t* hp = g_pin.p;
    uint32_t r = 0, longest = 0, plo = 0, phi = 0;
    bool seen = false;
    auto take = [&]() { r = hp[0]; longest = hp[1]; plo = hp[2]; phi = hp[3]; seen = true; };
    for (long spin = 0; ; spin++) {
        if (__atomic_load_n(&hp[4], __ATOMIC_ACQUIRE) == g_pin.seq) { take(); break; }
        if ((spin & 1023) == 1023) {
            if (hipEventQuery(g_pin.ev) != hipErrorNotReady) {
                // the plan's kernels are done (or the stream is in error): the stores are visible now, or they never will be
                if (__atomic_load_n(&hp[4], __ATOMIC_ACQUIRE) == g_pin.seq) take();
                break;
            }
            // earlier work still ahead of the plan on this stream (a caller that runs ahead): stop burning the core
            if (spin > (1l << 17)) { (void)hipEventSynchronize(g_pin.ev); if (__atomic_load_n(&hp[4], __ATOMIC_ACQUIRE) == g_pin.seq) take(); break; }
        }
        __builtin_ia32_pause();
    }
    if (!seen) {
        uint32_t tmp[4] = {0u, 0u, 0u, 0u};
        DM2_HIP(hipMemcpyAsync(tmp, plan_meta, sizeof(tmp), hipMemcpyDeviceToHost, st));
        DM2_HIP(hipStreamSynchronize(st));
        r = tmp[0]; longest = tmp[1]; plo = tmp[2]; phi = tmp[3];
    }
    *num_rendered = (int64_t)r;
    *max_tile_entries = (int64_t)longest;
    if (pair_bound) *pair_bound = (int64_t)(((uint64_t)phi << 32) | plo);
    if (longest == 0xFFFFFFFFu) { *num_rendered = 0; *max_tile_entries = 0; return fail("more than 2^31 - 1 (tile, face) pairs: render smaller patches"); }
    return 0;
}

int check_render_desc(const dm2_render_desc* d) {
    if (!d) return fail("null descriptor");
    if (d->B < 0 || d->P < 0 || d->F < 0 || d->W < 0 || d->H < 0) return fail("negative size in descriptor");
    if (d->aa_temperature < 0 || d->aa_temperature > 1) return fail("aa_temperature must be in the range [0, 1]");
    if (d->K < 0) return fail("len_oarea_buffer must be non-negative");
    const int64_t gx = (d->W + dm2::TILE - 1) / dm2::TILE, gy = (d->H + dm2::TILE - 1) / dm2::TILE;
    if (gx > 0xFFFF || gy > 0xFFFF) return fail("patch too large: more than 65535 tiles per axis");
    if (d->B > 65535) return fail("more than 65535 views per call");
    if ((int64_t)d->B * gx * gy >= (1ll << 31)) return fail("too many tiles");
    if (!(d->flags & DM2_FLAG_TABLES_FROM_IMAGE) && d->B > 0 && d->F > 0 && d->P > 0 &&
        (!d->aa_face_verts || !d->aa_face_edges || !d->aa_face_edges_iszero || !d->aa_face_edges_recip || !d->aa_face_edges_normal || !d->aa_face_edges_normal_c))
        return fail("the aa_face_* tables must not be null (or set DM2_FLAG_TABLES_FROM_IMAGE)");
    if (d->flags & DM2_FLAG_ANALYTIC_RAYS) {
        if (!d->ray_cam && d->B > 0) return fail("DM2_FLAG_ANALYTIC_RAYS needs ray_cam");
        if (d->full_W <= 0 || d->full_H <= 0) return fail("DM2_FLAG_ANALYTIC_RAYS needs the full image size");
    }
    return 0;
}

struct Profiler {
    bool on = false;
    hipEvent_t ev[2 * DM2_PROFILE_STAGES] = {};
    bool have[DM2_PROFILE_STAGES] = {};
    bool created = false;
};
thread_local Profiler g_prof;

inline int64_t tiles_of(int B, int W, int H) {
    return (int64_t)B * ((W + dm2::TILE - 1) / dm2::TILE) * ((H + dm2::TILE - 1) / dm2::TILE);
}

}  // namespace

namespace dm2 {
void prof_begin(int stage, hipStream_t st) {
    Profiler& p = g_prof;
    if (!p.on) return;
    if (!p.created) { for (auto& e : p.ev) (void)hipEventCreate(&e); p.created = true; }
    (void)hipEventRecord(p.ev[2 * stage], st);
}
void prof_end(int stage, hipStream_t st) {
    Profiler& p = g_prof;
    if (!p.on) return;
    (void)hipEventRecord(p.ev[2 * stage + 1], st);
    p.have[stage] = true;
}
}  // namespace dm2

extern "C" {

void dm2_profile_enable(int on) {
    g_prof.on = on != 0;
    for (auto& h : g_prof.have) h = false;
}

int dm2_profile_read(float* ms, int capacity) {
    Profiler& p = g_prof;
    int n = 0;
    for (int s = 0; s < DM2_PROFILE_STAGES && s < capacity; s++, n++) {
        ms[s] = 0.f;
        if (!p.on || !p.have[s]) continue;
        if (hipEventSynchronize(p.ev[2 * s + 1]) != hipSuccess) continue;
        float t = 0.f;
        if (hipEventElapsedTime(&t, p.ev[2 * s], p.ev[2 * s + 1]) == hipSuccess) ms[s] = t;
    }
    return n;
}

int dm2_debug_stamps(uint64_t* out, int capacity, int reset) {
#ifdef DM2_STAMPS
    unsigned long long h[2][DM2_NSTAMP];
    if (hipMemcpy(h, dm2::stamps_table(), sizeof(h), hipMemcpyDeviceToHost) != hipSuccess) return -2;
    int n = 0;
    for (int k = 0; k < 2; k++) for (int i = 0; i < DM2_NSTAMP && n < capacity; i++) out[n++] = h[k][i];
    if (reset) (void)hipMemset(dm2::stamps_table(), 0, sizeof(h));
    return n;
#else
    (void)out; (void)capacity; (void)reset;
    return -1;
#endif
}

int dm2_abi_version(void) { return DM2_ABI_VERSION; }
const char* dm2_last_error(void) { return g_err.c_str(); }

size_t dm2_scratch_bytes(int kind, int64_t count, int64_t aux) {
    size_t total = 0;
    if (count < 0) count = 0;
    if (aux < 0) aux = 0;
    switch (kind) {
        case DM2_SCRATCH_FACE: dm2::FaceState::carve(nullptr, count, aux >> 1, dm2::scan_temp_bytes(count), (aux & 1) != 0, &total); break;
        case DM2_SCRATCH_IMAGE: dm2::ImageState::carve(nullptr, count, aux, &total); break;
        case DM2_SCRATCH_BINNING: dm2::BinningState::carve(nullptr, count, dm2::sort_temp_bytes(count, aux), &total); break;
        case DM2_SCRATCH_LAYER_IMAGE: dm2::LayerImageState::carve(nullptr, count, aux, &total); break;
        case DM2_SCRATCH_LAYER_TETS: return dm2::tet_scratch_bytes(count);
        case DM2_SCRATCH_PAIR_POOL: return dm2::BinningState::pool_bytes(count);
        case DM2_SCRATCH_TIE_QUEUE: return count > 0 ? (size_t)count * sizeof(dm2::TieEntry) + dm2::ALIGN : 0;
        default: return 0;
    }
    return total;
}

static int forward_plan(const dm2_render_desc* d, void* face_scratch, size_t face_bytes, void* stream, int64_t* num_rendered,
                        int64_t* max_tile_entries, int64_t* pair_bound, uint2* ranges_to_clear, uint32_t* tile_order) {
    if (check_render_desc(d)) return 1;
    if (!num_rendered || !max_tile_entries) return fail("num_rendered / max_tile_entries is null");
    hipStream_t st = (hipStream_t)stream;
    const int64_t BF = (int64_t)d->B * d->F, Tn = tiles_of(d->B, d->W, d->H);
    *num_rendered = 0; *max_tile_entries = 0;
    if (pair_bound) *pair_bound = 0;
    if (d->P == 0 || BF == 0 || Tn == 0) return 0;                       // render.cu:149
    if (dm2_scratch_bytes(DM2_SCRATCH_FACE, BF, 2 * Tn + 1) > face_bytes) return fail("face scratch too small");
    dm2::FaceState fs = dm2::FaceState::carve(face_scratch, BF, Tn, dm2::scan_temp_bytes(BF), true);
    uint32_t* host_meta = nullptr; uint32_t seq = 0;
    if (plan_meta_prepare(&host_meta, &seq)) return 1;
    DM2_HIP(dm2::launch_preprocess_scan(d->B, d->P, d->F, d->W, d->H, d->patch_min, d->faces, d->verts_ndc, d->verts_image, fs, d,
                                        host_meta, seq, ranges_to_clear, tile_order, st));
    DM2_HIP(hipGetLastError());
    return plan_meta_wait(fs.plan_meta, st, num_rendered, max_tile_entries, pair_bound);
}

int dm2_forward_plan(const dm2_render_desc* d, void* face_scratch, size_t face_bytes, void* stream, int64_t* num_rendered,
                     int64_t* max_tile_entries, int64_t* pair_bound) {
    return forward_plan(d, face_scratch, face_bytes, stream, num_rendered, max_tile_entries, pair_bound, nullptr, nullptr);
}

static int forward_run(const dm2_render_desc* d, int64_t num_rendered, int64_t max_tile_entries, int64_t pair_bound, void* face_scratch, size_t face_bytes,
                       void* binning_scratch, size_t binning_bytes, void* image_scratch, size_t image_bytes,
                       float* out_color, float* out_depth, int32_t* out_tri_cnt, float* out_face_weights, void* stream,
                       bool ranges_cleared, int32_t* forward_mode) {
    if (forward_mode) *forward_mode = DM2_FWD_NONE;
    if (check_render_desc(d)) return 1;
    hipStream_t st = (hipStream_t)stream;
    const int64_t BF = (int64_t)d->B * d->F, N = (int64_t)d->B * d->H * d->W, Tn = tiles_of(d->B, d->W, d->H);
    if (N == 0) return 0;
    if (dm2_scratch_bytes(DM2_SCRATCH_IMAGE, N, Tn) > image_bytes) return fail("image scratch too small");
    dm2::ImageState is = dm2::ImageState::carve(image_scratch, N, Tn);
    const bool have_faces = (d->P != 0 && BF != 0);
    dm2::BinningState bs{};
    if (have_faces) {
        if (dm2_scratch_bytes(DM2_SCRATCH_FACE, BF, 2 * Tn + 1) > face_bytes) return fail("face scratch too small");
        if (dm2_scratch_bytes(DM2_SCRATCH_BINNING, num_rendered, Tn) > binning_bytes) return fail("binning scratch too small");
        dm2::FaceState fs = dm2::FaceState::carve(face_scratch, BF, Tn, dm2::scan_temp_bytes(BF), true);
        bs = dm2::BinningState::carve(binning_scratch, num_rendered, dm2::sort_temp_bytes(num_rendered, Tn), nullptr, binning_bytes);
        is.face_recs = fs.recs;
        DM2_HIP(dm2::launch_bin_sort(d->B, d->F, d->W, d->H, num_rendered, max_tile_entries, (d->flags & DM2_FLAG_LEGACY_KERNELS) != 0,
                                     fs.depths, fs, bs, is.ranges, ranges_cleared, is.tile_order, st));   // renderer.cu:192
    } else {
        DM2_HIP(hipMemsetAsync(is.ranges, 0, (size_t)Tn * sizeof(uint2), st));
        dm2::launch_tile_order_identity(Tn, is.tile_order, st);
    }
    // the pair pool is used when the caller appended room for every pair the plan counted (a smaller appendix is ignored)
    const bool use_pool = have_faces && pair_bound > 0 && bs.pool_cap >= pair_bound && !(d->flags & DM2_FLAG_NO_PAIR_POOL);
    const float pairs_per_entry = num_rendered > 0 ? (float)((double)pair_bound / (double)num_rendered) : 0.0f;
    const int mode = dm2::launch_render_forward(*d, is.ranges, bs.face_list, is, out_color, out_depth, out_tri_cnt, bs, use_pool, pairs_per_entry,
                                                out_face_weights, st);
    if (forward_mode) *forward_mode = mode;
    DM2_HIP(hipGetLastError());
    return 0;
}

int dm2_forward_run(const dm2_render_desc* d, int64_t num_rendered, int64_t max_tile_entries, int64_t pair_bound,
                    void* face_scratch, size_t face_bytes, void* binning_scratch, size_t binning_bytes,
                    void* image_scratch, size_t image_bytes, float* out_color, float* out_depth, int32_t* out_tri_cnt,
                    float* out_face_weights, void* stream, int32_t* forward_mode) {
    return forward_run(d, num_rendered, max_tile_entries, pair_bound, face_scratch, face_bytes, binning_scratch, binning_bytes, image_scratch,
                       image_bytes, out_color, out_depth, out_tri_cnt, out_face_weights, stream, false, forward_mode);
}

int dm2_forward(const dm2_render_desc* d, void* face_scratch, size_t face_bytes, void* binning_scratch, size_t binning_bytes,
                void* image_scratch, size_t image_bytes, float* out_color, float* out_depth, int32_t* out_tri_cnt,
                float* out_face_weights, void* stream, int64_t* num_rendered, int64_t* max_tile_entries, int64_t* pair_bound,
                int32_t* forward_mode) {
    if (check_render_desc(d)) return 1;
    if (!pair_bound) return fail("pair_bound is null");
    if (forward_mode) *forward_mode = DM2_FWD_NONE;
    const int64_t N = (int64_t)d->B * d->H * d->W, Tn = tiles_of(d->B, d->W, d->H);
    // the image scratch is at hand already: the plan's last kernel clears the tile ranges, one launch less in the run step
    uint2* ranges = nullptr; uint32_t* tile_order = nullptr;
    if (N > 0 && image_scratch && dm2_scratch_bytes(DM2_SCRATCH_IMAGE, N, Tn) <= image_bytes) {
        const dm2::ImageState is0 = dm2::ImageState::carve(image_scratch, N, Tn);
        ranges = is0.ranges; tile_order = is0.tile_order;
    }
    if (forward_plan(d, face_scratch, face_bytes, stream, num_rendered, max_tile_entries, pair_bound, ranges, tile_order)) return 1;
    const bool planned = d->P != 0 && (int64_t)d->B * d->F != 0 && Tn != 0;     // (otherwise no plan kernel ran)
    const bool wants_pool = d->aa_temperature > 0.0f && !(d->flags & (DM2_FLAG_NO_BACKWARD | DM2_FLAG_LEGACY_KERNELS | DM2_FLAG_NO_PAIR_POOL));
    if (dm2_scratch_bytes(DM2_SCRATCH_BINNING, *num_rendered, Tn) + (wants_pool ? dm2_scratch_bytes(DM2_SCRATCH_PAIR_POOL, *pair_bound, 0) : 0) > binning_bytes)
        return 2;                                                                // plan done; allocate, then dm2_forward_run
    return forward_run(d, *num_rendered, *max_tile_entries, *pair_bound, face_scratch, face_bytes, binning_scratch, binning_bytes,
                       image_scratch, image_bytes, out_color, out_depth, out_tri_cnt, out_face_weights, stream, planned && ranges != nullptr,
                       forward_mode);
}

int dm2_forward_alpha(const dm2_render_desc* d, const void* image_scratch, size_t image_bytes, float* out_alpha, void* stream) {
    if (check_render_desc(d)) return 1;
    const int64_t N = (int64_t)d->B * d->H * d->W, Tn = tiles_of(d->B, d->W, d->H);
    if (N == 0) return 0;
    if (!image_scratch || !out_alpha) return fail("image_scratch / out_alpha must not be null");
    if (dm2_scratch_bytes(DM2_SCRATCH_IMAGE, N, Tn) > image_bytes) return fail("image scratch too small");
    dm2::launch_forward_alpha(dm2::ImageState::carve(const_cast<void*>(image_scratch), N, Tn), N, out_alpha, (hipStream_t)stream);
    DM2_HIP(hipGetLastError());
    return 0;
}

int dm2_backward(const dm2_render_desc* d, int64_t num_rendered, int32_t forward_mode, const float* dL_dout_color,
                 const float* dL_dout_depth, const float* dL_dout_alpha,
                 const void* face_scratch, size_t face_bytes, void* binning_scratch, size_t binning_bytes,
                 const void* image_scratch, size_t image_bytes, void* tie_scratch, size_t tie_bytes,
                 float* dL_dverts, float* dL_dverts_color, float* dL_dfaces_opacity, float* dL_dverts_ndc,
                 float* dL_dfaces_intense, float* dL_daa_face_verts, void* stream) {
    if (check_render_desc(d)) return 1;
    hipStream_t st = (hipStream_t)stream;
    const int64_t N = (int64_t)d->B * d->H * d->W, Tn = tiles_of(d->B, d->W, d->H);
    if (d->F == 0 || d->P == 0 || N == 0 || num_rendered <= 0) return 0;       // render.cu:320
    const int64_t BF = (int64_t)d->B * d->F;
    if (dm2_scratch_bytes(DM2_SCRATCH_FACE, BF, 2 * Tn + 1) > face_bytes) return fail("face scratch too small");
    if (dm2_scratch_bytes(DM2_SCRATCH_IMAGE, N, Tn) > image_bytes) return fail("image scratch too small");
    if (dm2_scratch_bytes(DM2_SCRATCH_BINNING, num_rendered, Tn) > binning_bytes) return fail("binning scratch too small");
    dm2::ImageState is = dm2::ImageState::carve(const_cast<void*>(image_scratch), N, Tn);
    if (forward_mode < DM2_FWD_UNKNOWN || forward_mode > DM2_FWD_POINT) return fail("forward_mode must be one of DM2_FWD_*");
    dm2::BinningState bs = dm2::BinningState::carve(binning_scratch, num_rendered, dm2::sort_temp_bytes(num_rendered, Tn), nullptr, binning_bytes);
    is.face_recs = dm2::FaceState::carve(const_cast<void*>(face_scratch), BF, Tn, dm2::scan_temp_bytes(BF), true).recs;
    // the tie queue holds at most one entry per pair of the pool
    dm2::TieEntry* tie_queue = nullptr; int64_t tie_cap = 0;
    if (tie_scratch && tie_bytes >= sizeof(dm2::TieEntry) + dm2::ALIGN) {
        dm2::Carver c(tie_scratch);
        tie_queue = c.take<dm2::TieEntry>(0);
        tie_cap = (int64_t)((tie_bytes - c.used(tie_scratch)) / sizeof(dm2::TieEntry));
    }
    // the routes of dm2_backward.hip's table that reach the pool kernel: told DM2_FWD_POOL, or the cascade at temperature > 0
    const bool pool_route = d->aa_temperature > 0.0f && !(d->flags & DM2_FLAG_LEGACY_KERNELS) &&
                            (forward_mode == DM2_FWD_POOL || forward_mode == DM2_FWD_UNKNOWN || forward_mode == DM2_FWD_POINT);
    if (pool_route) {
        if (forward_mode == DM2_FWD_POOL && bs.pool_cap <= 0) return fail("forward_mode is DM2_FWD_POOL but the binning scratch has no pool part");
        if (tie_cap < bs.pool_cap) return fail("tie scratch too small for the pool part of the binning scratch");
    }
    dm2::launch_render_backward(*d, is.ranges, bs.face_list, is, dL_dout_color, dL_dout_depth, dL_dverts, dL_dverts_color,
                                dL_dfaces_opacity, dL_dverts_ndc, dL_dfaces_intense, dL_daa_face_verts, bs, forward_mode, tie_queue, tie_cap,
                                dL_dout_alpha, st);
    DM2_HIP(hipGetLastError());
    return 0;
}

static int check_layers_desc(const dm2_layers_desc* d) {
    if (!d) return fail("null descriptor");
    if (d->B < 0 || d->P < 0 || d->F < 0 || d->T < 0 || d->W < 0 || d->H < 0) return fail("negative size in descriptor");
    if (d->L < 0) return fail("num_layers must be non-negative");
    const int64_t gx = (d->W + dm2::TILE - 1) / dm2::TILE, gy = (d->H + dm2::TILE - 1) / dm2::TILE;
    if (gx > 0xFFFF || gy > 0xFFFF || d->B > 65535) return fail("image too large");
    if ((int64_t)d->B * gx * gy >= (1ll << 31)) return fail("too many tiles");
    if ((d->flags & DM2_FLAG_ANALYTIC_RAYS) && !d->ray_cam && d->B > 0) return fail("DM2_FLAG_ANALYTIC_RAYS needs ray_cam");
    return 0;
}

// The window a call works in: the caller's, or -- a null pointer -- the full frame of W x H at origin 0.  A window's origins
// are device memory: that it lies inside the frame is the caller's check (no kernel indexes memory through an origin).
static int resolve_window(const dm2_window* win, int W, int H, dm2_window* out) {
    if (!win) { *out = dm2_window{nullptr, W, H}; return 0; }
    if (win->full_W < W || win->full_H < H) return fail("window: full_W / full_H must hold the window's W / H");
    *out = *win;
    return 0;
}

int dm2_layers_plan(const dm2_layers_desc* d, const dm2_window* win, void* face_scratch, size_t face_bytes, void* stream,
                    int64_t* num_rendered, int64_t* max_tile_entries) {
    if (check_layers_desc(d)) return 1;
    dm2_window w;
    if (resolve_window(win, d->W, d->H, &w)) return 1;
    if (!num_rendered || !max_tile_entries) return fail("num_rendered / max_tile_entries is null");
    hipStream_t st = (hipStream_t)stream;
    const int64_t BF = (int64_t)d->B * d->F, Tn = tiles_of(d->B, d->W, d->H);
    *num_rendered = 0; *max_tile_entries = 0;
    if (BF == 0 || Tn == 0) return 0;
    if (dm2_scratch_bytes(DM2_SCRATCH_FACE, BF, 2 * Tn) > face_bytes) return fail("face scratch too small");
    dm2::FaceState fs = dm2::FaceState::carve(face_scratch, BF, Tn, dm2::scan_temp_bytes(BF), false);
    // the full frame: patch_min = 0 (renderer.cu:557-558), a null patch_min means "all zeros"; a window: its origins, and the
    // tiles of its W x H
    uint32_t* host_meta = nullptr; uint32_t seq = 0;
    if (plan_meta_prepare(&host_meta, &seq)) return 1;
    DM2_HIP(dm2::launch_preprocess_scan(d->B, d->P, d->F, d->W, d->H, w.patch_min, d->faces, d->verts_ndc, d->verts_image, fs, nullptr,
                                        host_meta, seq, nullptr, nullptr, st));
    DM2_HIP(hipGetLastError());
    return plan_meta_wait(fs.plan_meta, st, num_rendered, max_tile_entries, nullptr);
}

// The binning step of dm2_layers_run and dm2_rasterize_run: the tile lists of a dm2_layers_plan, ordered by min depth, and their
// ranges (all empty without faces, where nothing was planned).
static int layers_bin_sort(const dm2_layers_desc* d, int64_t num_rendered, int64_t max_tile_entries, void* face_scratch,
                           size_t face_bytes, void* binning_scratch, size_t binning_bytes, uint2* ranges, dm2::FaceState* fs,
                           dm2::BinningState* bs, hipStream_t st) {
    const int64_t BF = (int64_t)d->B * d->F, Tn = tiles_of(d->B, d->W, d->H);
    if (BF != 0) {
        if (dm2_scratch_bytes(DM2_SCRATCH_FACE, BF, 2 * Tn) > face_bytes) return fail("face scratch too small");
        if (dm2_scratch_bytes(DM2_SCRATCH_BINNING, num_rendered, Tn) > binning_bytes) return fail("binning scratch too small");
        *fs = dm2::FaceState::carve(face_scratch, BF, Tn, dm2::scan_temp_bytes(BF), false);
        *bs = dm2::BinningState::carve(binning_scratch, num_rendered, dm2::sort_temp_bytes(num_rendered, Tn));
        DM2_HIP(dm2::launch_bin_sort(d->B, d->F, d->W, d->H, num_rendered, max_tile_entries, (d->flags & DM2_FLAG_LEGACY_KERNELS) != 0,
                                     fs->min_depths, *fs, *bs, ranges, false, nullptr, st));   // renderer.cu:603
    } else {
        DM2_HIP(hipMemsetAsync(ranges, 0, (size_t)Tn * sizeof(uint2), st));
    }
    return 0;
}

int dm2_layers_run(const dm2_layers_desc* d, const dm2_window* win, int64_t num_rendered, int64_t max_tile_entries,
                   void* face_scratch, size_t face_bytes, void* binning_scratch, size_t binning_bytes,
                   void* image_scratch, size_t image_bytes, void* tet_scratch, size_t tet_bytes,
                   int32_t* render_layers, int32_t* render_layers_cnt, void* stream) {
    if (check_layers_desc(d)) return 1;
    dm2_window w;
    if (resolve_window(win, d->W, d->H, &w)) return 1;
    hipStream_t st = (hipStream_t)stream;
    const int64_t N = (int64_t)d->B * d->H * d->W, Tn = tiles_of(d->B, d->W, d->H);
    if (N == 0) return 0;
    if (dm2_scratch_bytes(DM2_SCRATCH_LAYER_IMAGE, N, Tn) > image_bytes) return fail("image scratch too small");
    dm2::LayerImageState ls = dm2::LayerImageState::carve(image_scratch, N, Tn);
    dm2::FaceState fs{};
    dm2::BinningState bs{};
    if (layers_bin_sort(d, num_rendered, max_tile_entries, face_scratch, face_bytes, binning_scratch, binning_bytes, ls.ranges, &fs, &bs, st))
        return 1;
    if (tet_scratch && dm2_scratch_bytes(DM2_SCRATCH_LAYER_TETS, d->T, 0) > tet_bytes) return fail("tet scratch too small");
    dm2::launch_layers(*d, w, fs, ls.ranges, bs.face_list, ls, tet_scratch, render_layers, render_layers_cnt, st);
    DM2_HIP(hipGetLastError());
    return 0;
}

static int check_rasterize_inputs(const dm2_layers_desc* d) {
    if (d->F > 0 && d->B > 0 && (!d->verts || !d->faces)) return fail("verts / faces must not be null");
    if (!(d->flags & DM2_FLAG_ANALYTIC_RAYS) && d->B > 0 && (!d->image_ray_o || !d->image_ray_d))
        return fail("image_ray_o / image_ray_d must not be null");
    return 0;
}

// overlap == 0 (`inside` is not looked at) and overlap != 0: the same plan, scratch and tile lists; only the kernel over the
// lists differs.
int dm2_rasterize_run(const dm2_layers_desc* d, const dm2_window* win, int64_t num_rendered, int64_t max_tile_entries,
                      void* face_scratch, size_t face_bytes, void* binning_scratch, size_t binning_bytes,
                      void* image_scratch, size_t image_bytes, int32_t* render_layers, int32_t* render_layers_cnt,
                      float* bary, float* t, int32_t overlap, uint8_t* inside, void* stream) {
    if (check_layers_desc(d) || check_rasterize_inputs(d)) return 1;
    dm2_window w;
    if (resolve_window(win, d->W, d->H, &w)) return 1;
    hipStream_t st = (hipStream_t)stream;
    const int64_t N = (int64_t)d->B * d->H * d->W, Tn = tiles_of(d->B, d->W, d->H);
    if (N == 0) return 0;
    if (!render_layers_cnt || (d->L > 0 && (!render_layers || !bary || !t))) return fail("rasterize outputs must not be null");
    if (overlap && d->L > 0 && !inside) return fail("rasterize (overlap): inside must not be null");
    if (overlap && d->L > 0 && d->F > 0 && !d->verts_image) return fail("rasterize (overlap): verts_image must not be null");
    if (d->L == 0) {
        DM2_HIP(hipMemsetAsync(render_layers_cnt, 0, (size_t)N * sizeof(int32_t), st));
        return 0;
    }
    if (dm2_scratch_bytes(DM2_SCRATCH_LAYER_IMAGE, N, Tn) > image_bytes) return fail("image scratch too small");
    dm2::LayerImageState ls = dm2::LayerImageState::carve(image_scratch, N, Tn);
    dm2::FaceState fs{};
    dm2::BinningState bs{};
    if (layers_bin_sort(d, num_rendered, max_tile_entries, face_scratch, face_bytes, binning_scratch, binning_bytes, ls.ranges, &fs, &bs, st))
        return 1;
    if (overlap) dm2::launch_rasterize_overlap(*d, w, ls.ranges, bs.face_list, render_layers, render_layers_cnt, bary, t, inside, st);
    else dm2::launch_rasterize(*d, w, fs, ls.ranges, bs.face_list, render_layers, render_layers_cnt, bary, t, st);
    DM2_HIP(hipGetLastError());
    return 0;
}

int dm2_rasterize_backward(const dm2_layers_desc* d, const dm2_window* win, const int32_t* render_layers, const float* dL_dbary,
                           const float* dL_dt, float* dL_dverts, int32_t overlap, void* stream) {
    if (check_layers_desc(d) || check_rasterize_inputs(d)) return 1;
    dm2_window w;
    if (resolve_window(win, d->W, d->H, &w)) return 1;
    if ((int64_t)d->B * d->H * d->W == 0 || d->L == 0 || d->F == 0 || (!dL_dbary && !dL_dt)) return 0;   // nothing is listed or nothing flows
    if (!render_layers || !dL_dverts) return fail("render_layers / dL_dverts must not be null");
    if (overlap) dm2::launch_rasterize_overlap_backward(*d, w, render_layers, dL_dbary, dL_dt, dL_dverts, (hipStream_t)stream);
    else dm2::launch_rasterize_backward(*d, w, render_layers, dL_dbary, dL_dt, dL_dverts, (hipStream_t)stream);
    DM2_HIP(hipGetLastError());
    return 0;
}

static int check_interpolate_sizes(int32_t B, int32_t H, int32_t W, int32_t L, int32_t F, int32_t N, int32_t C, int32_t view_tables) {
    if (B < 0 || H < 0 || W < 0 || L < 0 || F < 0 || N < 0) return fail("interpolate: negative size");
    if (C < 1) return fail("interpolate: C must be at least 1");
    if (view_tables && (int64_t)B * N > 0x7FFFFFFF) return fail("interpolate: B * N must be below 2^31");
    // (the attr backward's grid is one block per tile and view: tile rows and views are grid dimensions of 16 bits)
    if (((int64_t)B * H * W * L + 255) / 256 > 0x7FFFFFFF || B > 65535 || ((int64_t)H + dm2::TILE - 1) / dm2::TILE > 65535)
        return fail("interpolate: too many slots, rows or views");
    return 0;
}

int dm2_interpolate(int32_t B, int32_t H, int32_t W, int32_t L, int32_t F, int32_t N, int32_t C, int32_t view_tables,
                    const int32_t* render_layers, const float* bary, const float* attr, const int32_t* attr_faces,
                    float* out, void* stream) {
    if (check_interpolate_sizes(B, H, W, L, F, N, C, view_tables)) return 1;
    const int64_t S = (int64_t)B * H * W * L;
    if (S == 0) return 0;
    if (!out) return fail("interpolate: out must not be null");
    if (F == 0 || N == 0) {                                              // every slot is empty
        DM2_HIP(hipMemsetAsync(out, 0, (size_t)S * C * sizeof(float), (hipStream_t)stream));
        return 0;
    }
    if (!render_layers || !bary || !attr || !attr_faces) return fail("interpolate: inputs must not be null");
    dm2::launch_interpolate(B, H, W, L, F, N, C, view_tables, render_layers, bary, attr, attr_faces, out, (hipStream_t)stream);
    DM2_HIP(hipGetLastError());
    return 0;
}

int dm2_interpolate_backward(int32_t B, int32_t H, int32_t W, int32_t L, int32_t F, int32_t N, int32_t C, int32_t view_tables,
                             const int32_t* render_layers, const float* bary, const float* attr, const int32_t* attr_faces,
                             const float* dL_dout, float* dL_dattr, float* dL_dbary, void* stream) {
    if (check_interpolate_sizes(B, H, W, L, F, N, C, view_tables)) return 1;
    const int64_t S = (int64_t)B * H * W * L;
    if (S == 0 || (!dL_dattr && !dL_dbary)) return 0;
    if (F == 0 || N == 0) {                                              // every slot is empty: nothing reaches attr
        if (dL_dbary) DM2_HIP(hipMemsetAsync(dL_dbary, 0, (size_t)S * 3 * sizeof(float), (hipStream_t)stream));
        return 0;
    }
    if (!render_layers || !attr_faces || !dL_dout) return fail("interpolate_backward: inputs must not be null");
    if (dL_dattr && !bary) return fail("interpolate_backward: bary must not be null");
    if (dL_dbary && !attr) return fail("interpolate_backward: attr must not be null");
    dm2::launch_interpolate_backward(B, H, W, L, F, N, C, view_tables, render_layers, bary, attr, attr_faces, dL_dout, dL_dattr,
                                     dL_dbary, (hipStream_t)stream);
    DM2_HIP(hipGetLastError());
    return 0;
}

// The launch bound the lookup ops share: 256 slots per block, one grid row per view (hash grid: per view and level).
static int check_slot_grid(const char* op, int64_t S, int64_t views, int64_t H) {
    if ((S + 255) / 256 > 0x7FFFFFFF || views > 65535 || (H + dm2::TILE - 1) / dm2::TILE > 65535)
        return fail(std::string(op) + ": too many slots, rows or views");
    return 0;
}

// A nearest filter is piecewise constant in the coordinate: its gradient, S * k floats, is zeroed on the stream and dropped.
static int zero_nearest_grad(int filter, float** grad, int64_t S, int k, void* stream) {
    if (!*grad || filter != DM2_TEX_FILTER_NEAREST) return 0;
    DM2_HIP(hipMemsetAsync(*grad, 0, (size_t)S * k * sizeof(float), (hipStream_t)stream));
    *grad = nullptr;
    return 0;
}

static int check_texture_sizes(int32_t B, int32_t H, int32_t W, int32_t L, int32_t Ht, int32_t Wt, int32_t C, int32_t filter,
                               int32_t boundary) {
    if (B < 0 || H < 0 || W < 0 || L < 0) return fail("texture: negative size");
    if (Ht < 1 || Wt < 1) return fail("texture: Ht and Wt must be at least 1");
    if ((int64_t)Ht * Wt > 0x7FFFFFFF) return fail("texture: Ht * Wt must be below 2^31");
    if (C < 1) return fail("texture: C must be at least 1");
    if (filter != DM2_TEX_FILTER_NEAREST && filter != DM2_TEX_FILTER_LINEAR) return fail("texture: unknown filter");
    if (boundary != DM2_TEX_BOUNDARY_WRAP && boundary != DM2_TEX_BOUNDARY_CLAMP) return fail("texture: unknown boundary");
    return check_slot_grid("texture", (int64_t)B * H * W * L, B, H);
}

int dm2_texture(int32_t B, int32_t H, int32_t W, int32_t L, int32_t Ht, int32_t Wt, int32_t C, int32_t view_textures,
                int32_t filter, int32_t boundary, const int32_t* render_layers, const float* uv, const float* tex, float* out,
                void* stream) {
    if (check_texture_sizes(B, H, W, L, Ht, Wt, C, filter, boundary)) return 1;
    if ((int64_t)B * H * W * L == 0) return 0;
    if (!uv || !tex || !out) return fail("texture: uv, tex and out must not be null");
    dm2::launch_texture(B, H, W, L, Ht, Wt, C, view_textures, filter, boundary, render_layers, uv, tex, out, (hipStream_t)stream);
    DM2_HIP(hipGetLastError());
    return 0;
}

int dm2_texture_backward(int32_t B, int32_t H, int32_t W, int32_t L, int32_t Ht, int32_t Wt, int32_t C, int32_t view_textures,
                         int32_t filter, int32_t boundary, const int32_t* render_layers, const float* uv, const float* tex,
                         const float* dL_dout, float* dL_dtex, float* dL_duv, void* stream) {
    if (check_texture_sizes(B, H, W, L, Ht, Wt, C, filter, boundary)) return 1;
    const int64_t S = (int64_t)B * H * W * L;
    if (S == 0 || (!dL_dtex && !dL_duv)) return 0;
    if (!uv || !dL_dout) return fail("texture_backward: uv and dL_dout must not be null");
    if (zero_nearest_grad(filter, &dL_duv, S, 2, stream)) return 1;
    if (dL_duv && !tex) return fail("texture_backward: tex must not be null");
    if (dL_dtex || dL_duv)
        dm2::launch_texture_backward(B, H, W, L, Ht, Wt, C, view_textures, filter, boundary, render_layers, uv, tex, dL_dout,
                                     dL_dtex, dL_duv, (hipStream_t)stream);
    DM2_HIP(hipGetLastError());
    return 0;
}

// the sizes of a lookup into a table with faces or planes of N x N (op: the prefix of the messages)
static int check_texture_cube_sizes(const char* op, int32_t B, int32_t H, int32_t W, int32_t L, int32_t N, int32_t C, int32_t filter) {
    if (B < 0 || H < 0 || W < 0 || L < 0) return fail(std::string(op) + ": negative size");
    if (N < 1) return fail(std::string(op) + ": N must be at least 1");
    if ((int64_t)6 * N * N > 0x7FFFFFFF) return fail(std::string(op) + ": 6 * N * N must be below 2^31");
    if (C < 1) return fail(std::string(op) + ": C must be at least 1");
    if (filter != DM2_TEX_FILTER_NEAREST && filter != DM2_TEX_FILTER_LINEAR) return fail(std::string(op) + ": unknown filter");
    return check_slot_grid(op, (int64_t)B * H * W * L, B, H);
}

static int check_texture_volume_sizes(int32_t B, int32_t H, int32_t W, int32_t L, int32_t N, int32_t C, int32_t filter, int32_t boundary) {
    if (boundary != DM2_TEX_BOUNDARY_WRAP && boundary != DM2_TEX_BOUNDARY_CLAMP) return fail("texture_volume: unknown boundary");
    if (N > 1290) return fail("texture_volume: a volume's N * N * N must be below 2^31");     // 1290^3 < 2^31 < 1291^3
    return check_texture_cube_sizes("texture_volume", B, H, W, L, N, C, filter);              // (its own bound on N lies above this one)
}

int dm2_texture_volume(int32_t B, int32_t H, int32_t W, int32_t L, int32_t N, int32_t C, int32_t view_textures, int32_t filter,
                       int32_t boundary, const int32_t* render_layers, const float* xyz, const float* grid, float* out, void* stream) {
    if (check_texture_volume_sizes(B, H, W, L, N, C, filter, boundary)) return 1;
    if ((int64_t)B * H * W * L == 0) return 0;
    if (!xyz || !grid || !out) return fail("texture_volume: a volume's xyz, grid and out must not be null");
    dm2::launch_texture_volume(B, H, W, L, N, C, view_textures, filter, boundary, render_layers, xyz, grid, out, (hipStream_t)stream);
    DM2_HIP(hipGetLastError());
    return 0;
}

int dm2_texture_volume_backward(int32_t B, int32_t H, int32_t W, int32_t L, int32_t N, int32_t C, int32_t view_textures,
                                int32_t filter, int32_t boundary, const int32_t* render_layers, const float* xyz, const float* grid,
                                const float* dL_dout, float* dL_dgrid, float* dL_dxyz, void* stream) {
    if (check_texture_volume_sizes(B, H, W, L, N, C, filter, boundary)) return 1;
    const int64_t S = (int64_t)B * H * W * L;
    if (S == 0 || (!dL_dgrid && !dL_dxyz)) return 0;
    if (!xyz || !dL_dout) return fail("texture_volume_backward: a volume's xyz and dL_dout must not be null");
    if (zero_nearest_grad(filter, &dL_dxyz, S, 3, stream)) return 1;
    if (dL_dxyz && !grid) return fail("texture_volume_backward: a volume's grid must not be null");
    if (dL_dgrid || dL_dxyz)
        dm2::launch_texture_volume_backward(B, H, W, L, N, C, view_textures, filter, boundary, render_layers, xyz, grid, dL_dout,
                                            dL_dgrid, dL_dxyz, (hipStream_t)stream);
    DM2_HIP(hipGetLastError());
    return 0;
}

// R[l]: the level resolutions, R_0 = base_resolution, R_{l+1} = (R_l * growth16) >> 4
static int check_hash_grid(int32_t B, int32_t H, int32_t W, int32_t L, int32_t base_resolution, int32_t log2_rows, int32_t num_levels,
                           int32_t features, int32_t growth16, int32_t filter, int32_t boundary, int R[32]) {
    if (filter != DM2_TEX_FILTER_NEAREST && filter != DM2_TEX_FILTER_LINEAR) return fail("hash_grid: unknown filter");
    if (boundary != DM2_TEX_BOUNDARY_WRAP && boundary != DM2_TEX_BOUNDARY_CLAMP) return fail("hash_grid: unknown boundary");
    if (num_levels < 1 || num_levels > 32) return fail("hash_grid: a hash grid's num_levels must be in 1..32");
    if (growth16 < 17 || growth16 > 32) return fail("hash_grid: a hash grid's growth16 must be in 17..32");
    if (log2_rows < 4 || log2_rows > 24) return fail("hash_grid: a hash grid's log2(T) must be in 4..24");
    if (B < 0 || H < 0 || W < 0 || L < 0) return fail("hash_grid: negative size");
    if (base_resolution < 1) return fail("hash_grid: a hash grid's base resolution must be at least 1");
    if (features != 1 && features != 2 && features != 4 && features != 8) return fail("hash_grid: a hash grid's F must be 1, 2, 4 or 8");
    if (((int64_t)num_levels * features << log2_rows) > 0x7FFFFFFF) return fail("hash_grid: a hash grid's NL * T * F must be below 2^31");
    int64_t r = base_resolution;
    for (int l = 0; l < num_levels; l++) {
        if (r > (1 << 20)) return fail("hash_grid: a hash grid's finest resolution must not exceed 2^20");
        R[l] = (int)r;
        r = (r * growth16) >> 4;
    }
    return check_slot_grid("hash_grid", (int64_t)B * H * W * L, (int64_t)B * num_levels, H);
}

int dm2_hash_grid(int32_t B, int32_t H, int32_t W, int32_t L, int32_t base_resolution, int32_t log2_rows, int32_t num_levels,
                  int32_t features, int32_t growth16, int32_t filter, int32_t boundary, const int32_t* render_layers, const float* xyz,
                  const float* table, float* out, void* stream) {
    int R[32];
    if (check_hash_grid(B, H, W, L, base_resolution, log2_rows, num_levels, features, growth16, filter, boundary, R)) return 1;
    if (!xyz) return fail("hash_grid: a hash grid's xyz must not be null");
    if ((int64_t)B * H * W * L == 0) return 0;
    if (!table || !out) return fail("hash_grid: a hash grid's table and out must not be null");
    dm2::launch_hash_grid(B, H, W, L, num_levels, 1 << log2_rows, features, R, filter, boundary, render_layers, xyz, table, out,
                          (hipStream_t)stream);
    DM2_HIP(hipGetLastError());
    return 0;
}

int dm2_hash_grid_backward(int32_t B, int32_t H, int32_t W, int32_t L, int32_t base_resolution, int32_t log2_rows, int32_t num_levels,
                           int32_t features, int32_t growth16, int32_t filter, int32_t boundary, const int32_t* render_layers,
                           const float* xyz, const float* table, const float* dL_dout, float* dL_dtable, float* dL_dxyz, void* stream) {
    int R[32];
    if (check_hash_grid(B, H, W, L, base_resolution, log2_rows, num_levels, features, growth16, filter, boundary, R)) return 1;
    if (!xyz) return fail("hash_grid_backward: a hash grid's xyz must not be null");
    const int64_t S = (int64_t)B * H * W * L;
    if (S == 0 || (!dL_dtable && !dL_dxyz)) return 0;
    if (!dL_dout) return fail("hash_grid_backward: a hash grid's dL_dout must not be null");
    if (zero_nearest_grad(filter, &dL_dxyz, S, 3, stream)) return 1;
    if (dL_dxyz && !table) return fail("hash_grid_backward: a hash grid's table must not be null");
    if (dL_dtable || dL_dxyz)
        dm2::launch_hash_grid_backward(B, H, W, L, num_levels, 1 << log2_rows, features, R, filter, boundary, render_layers, xyz, table,
                                       dL_dout, dL_dtable, dL_dxyz, (hipStream_t)stream);
    DM2_HIP(hipGetLastError());
    return 0;
}

int dm2_texture_cube(int32_t B, int32_t H, int32_t W, int32_t L, int32_t N, int32_t C, int32_t view_textures, int32_t filter,
                     const int32_t* render_layers, const float* dirs, const float* tex, float* out, void* stream) {
    if (check_texture_cube_sizes("texture_cube", B, H, W, L, N, C, filter)) return 1;
    if ((int64_t)B * H * W * L == 0) return 0;
    if (!dirs || !tex || !out) return fail("texture_cube: dirs, tex and out must not be null");
    dm2::launch_texture_cube(B, H, W, L, N, C, view_textures, filter, render_layers, dirs, tex, out, (hipStream_t)stream);
    DM2_HIP(hipGetLastError());
    return 0;
}

int dm2_texture_cube_backward(int32_t B, int32_t H, int32_t W, int32_t L, int32_t N, int32_t C, int32_t view_textures,
                              int32_t filter, const int32_t* render_layers, const float* dirs, const float* tex,
                              const float* dL_dout, float* dL_dtex, float* dL_ddir, void* stream) {
    if (check_texture_cube_sizes("texture_cube", B, H, W, L, N, C, filter)) return 1;
    const int64_t S = (int64_t)B * H * W * L;
    if (S == 0 || (!dL_dtex && !dL_ddir)) return 0;
    if (!dirs || !dL_dout) return fail("texture_cube_backward: dirs and dL_dout must not be null");
    if (zero_nearest_grad(filter, &dL_ddir, S, 3, stream)) return 1;
    if (dL_ddir && !tex) return fail("texture_cube_backward: tex must not be null");
    if (dL_dtex || dL_ddir)
        dm2::launch_texture_cube_backward(B, H, W, L, N, C, view_textures, filter, render_layers, dirs, tex, dL_dout, dL_dtex,
                                          dL_ddir, (hipStream_t)stream);
    DM2_HIP(hipGetLastError());
    return 0;
}

int dm2_bary_derivatives_window(int32_t B, int32_t H, int32_t W, int32_t L, int32_t P, int32_t F, const dm2_window* win,
                                const int32_t* render_layers, const float* verts, const int32_t* faces, const float* ray_cam,
                                float* dbary_dx, float* dbary_dy, void* stream) {
    if (B < 0 || H < 0 || W < 0 || L < 0 || P < 0 || F < 0) return fail("bary_derivatives: negative size");
    const int64_t per_view = (int64_t)H * W * L;
    if (B > 65535 || (per_view + 255) / 256 > 0x7FFFFFFF) return fail("bary_derivatives: too many slots or views");
    if (win && (win->full_W < W || win->full_H < H)) return fail("bary_derivatives: the window is larger than its frame");
    const int64_t S = (int64_t)B * per_view;
    if (S == 0) return 0;
    if (!dbary_dx || !dbary_dy) return fail("bary_derivatives: the outputs must not be null");
    if (F == 0 || P == 0) {                                              // every slot is empty
        DM2_HIP(hipMemsetAsync(dbary_dx, 0, (size_t)S * 3 * sizeof(float), (hipStream_t)stream));
        DM2_HIP(hipMemsetAsync(dbary_dy, 0, (size_t)S * 3 * sizeof(float), (hipStream_t)stream));
        return 0;
    }
    if (!render_layers || !verts || !faces || !ray_cam) return fail("bary_derivatives: inputs must not be null");
    dm2::launch_bary_derivatives(B, H, W, L, P, F, win ? win->full_W : W, win ? win->full_H : H, win ? win->patch_min : nullptr,
                                 render_layers, verts, faces, ray_cam, dbary_dx, dbary_dy, (hipStream_t)stream);
    DM2_HIP(hipGetLastError());
    return 0;
}

static int check_vertex_normals(int32_t P, int32_t F, const void* scratch, size_t scratch_bytes, int backward) {
    if (P < 0 || F < 0) return fail("vertex_normals: negative size");
    if ((int64_t)3 * F > 0x7FFFFFFF) return fail("vertex_normals: 3 * F must be below 2^31");
    if (P == 0) return 0;
    const size_t need = dm2::vertex_normals_scratch_bytes(P, F, backward);
    if (F > 0 && (!scratch || scratch_bytes < need)) return fail("vertex_normals: scratch is smaller than dm2_vertex_normals_scratch_bytes");
    if ((uintptr_t)scratch % 16) return fail("vertex_normals: scratch must be 16-byte aligned");
    return 0;
}

size_t dm2_vertex_normals_scratch_bytes(int32_t P, int32_t F, int32_t backward) {
    if (P < 0 || F < 0) return 0;
    return dm2::vertex_normals_scratch_bytes(P, F, backward);
}

int dm2_vertex_normals(int32_t P, int32_t F, int32_t normalize, const float* verts, const int32_t* faces, const int32_t* offsets,
                       const int32_t* corners, void* scratch, size_t scratch_bytes, float* out_normals, float* out_len, void* stream) {
    if (check_vertex_normals(P, F, scratch, scratch_bytes, 0)) return 1;
    if (P == 0) return 0;
    if (!out_normals) return fail("vertex_normals: out_normals must not be null");
    if (!offsets) return fail("vertex_normals: offsets must not be null");
    if (F > 0 && (!verts || !faces || !corners)) return fail("vertex_normals: verts, faces and corners must not be null");
    dm2::launch_vertex_normals(P, F, normalize, verts, faces, offsets, corners, scratch, out_normals, out_len, (hipStream_t)stream);
    DM2_HIP(hipGetLastError());
    return 0;
}

int dm2_vertex_normals_backward(int32_t P, int32_t F, int32_t normalize, const float* verts, const int32_t* faces,
                                const int32_t* offsets, const int32_t* corners, const float* normals, const float* len,
                                const float* dL_dnormals, void* scratch, size_t scratch_bytes, float* dL_dverts, void* stream) {
    if (check_vertex_normals(P, F, scratch, scratch_bytes, 1)) return 1;
    if (P == 0 || !dL_dverts || !dL_dnormals) return 0;
    if (!offsets) return fail("vertex_normals_backward: offsets must not be null");
    if (F > 0 && (!verts || !faces || !corners)) return fail("vertex_normals_backward: verts, faces and corners must not be null");
    if (F > 0 && normalize && (!normals || !len)) return fail("vertex_normals_backward: normals and len must not be null");
    dm2::launch_vertex_normals_backward(P, F, normalize, verts, faces, offsets, corners, normals, len, dL_dnormals, scratch, dL_dverts,
                                        (hipStream_t)stream);
    DM2_HIP(hipGetLastError());
    return 0;
}

static int check_shading(int32_t B, int32_t H, int32_t W, int32_t L, int32_t flags, const dm2_window* win, const int32_t* render_layers,
                         const float* t, const float* image_ray_o, const float* image_ray_d, const float* ray_cam) {
    if (B < 0 || H < 0 || W < 0 || L < 0) return fail("shading_vectors: negative size");
    const int64_t per_view = (int64_t)H * W * L;
    if (B > 65535 || (per_view + 255) / 256 > 0x7FFFFFFF) return fail("shading_vectors: too many slots or views");
    if (flags & ~DM2_FLAG_ANALYTIC_RAYS) return fail("shading_vectors: unknown flag");
    if (win && (win->full_W < W || win->full_H < H)) return fail("shading_vectors: the window is larger than its frame");
    if ((int64_t)B * per_view == 0) return 0;
    if (!render_layers || !t) return fail("shading_vectors: render_layers and t must not be null");
    if (flags & DM2_FLAG_ANALYTIC_RAYS) {
        if (!ray_cam) return fail("shading_vectors: ray_cam must not be null");
    } else if (!image_ray_o || !image_ray_d) {
        return fail("shading_vectors: image_ray_o and image_ray_d must not be null");
    }
    return 0;
}

int dm2_shading_vectors_window(int32_t B, int32_t H, int32_t W, int32_t L, int32_t flags, const dm2_window* win,
                               const int32_t* render_layers, const float* t, const float* normals, const float* image_ray_o,
                               const float* image_ray_d, const float* ray_cam, float* out_position, float* out_view, float* out_normal,
                               float* out_reflection, void* stream) {
    if (check_shading(B, H, W, L, flags, win, render_layers, t, image_ray_o, image_ray_d, ray_cam)) return 1;
    if ((int64_t)B * H * W * L == 0) return 0;
    if (!out_position || !out_view) return fail("shading_vectors: out_position and out_view must not be null");
    if (normals && (!out_normal || !out_reflection)) return fail("shading_vectors: out_normal and out_reflection must not be null");
    dm2::launch_shading_vectors(B, H, W, L, flags, win ? win->full_W : W, win ? win->full_H : H, win ? win->patch_min : nullptr,
                                render_layers, t, normals, image_ray_o, image_ray_d, ray_cam, out_position, out_view, out_normal,
                                out_reflection, (hipStream_t)stream);
    DM2_HIP(hipGetLastError());
    return 0;
}

int dm2_shading_vectors_backward_window(int32_t B, int32_t H, int32_t W, int32_t L, int32_t flags, const dm2_window* win,
                                        const int32_t* render_layers, const float* t, const float* normals, const float* image_ray_o,
                                        const float* image_ray_d, const float* ray_cam, const float* g_position, const float* g_normal,
                                        const float* g_reflection, float* dL_dt, float* dL_dnormals, void* stream) {
    if (check_shading(B, H, W, L, flags, win, render_layers, t, image_ray_o, image_ray_d, ray_cam)) return 1;
    if ((int64_t)B * H * W * L == 0 || (!dL_dt && !dL_dnormals)) return 0;
    if (dL_dnormals && !normals) return fail("shading_vectors_backward: normals must not be null");
    dm2::launch_shading_vectors_backward(B, H, W, L, flags, win ? win->full_W : W, win ? win->full_H : H,
                                         win ? win->patch_min : nullptr, render_layers, t, normals, image_ray_o, image_ray_d, ray_cam,
                                         g_position, g_normal, g_reflection, dL_dt, dL_dnormals, (hipStream_t)stream);
    DM2_HIP(hipGetLastError());
    return 0;
}

// the chain of (Ht, Wt, C) under max_mip_level: sizes that the kernels' 32-bit texel indices and launch grids hold
static int check_mip_sizes(int32_t NB, int32_t Ht, int32_t Wt, int32_t C, int32_t max_mip_level, int64_t* T) {
    if (NB < 0 || NB > 65535) return fail("texture_mip: the number of textures must lie in [0, 65535]");
    if (Ht < 1 || Wt < 1) return fail("texture_mip: Ht and Wt must be at least 1");
    if (C < 1) return fail("texture_mip: C must be at least 1");
    dm2::mip_levels(Ht, Wt, max_mip_level, T);
    if ((int64_t)Ht * Wt + *T > 0x7FFFFFFF) return fail("texture_mip: the texels of all levels must number below 2^31");
    if (((int64_t)Ht * Wt * C + 255) / 256 > 0x7FFFFFFF) return fail("texture_mip: texture too large");
    return 0;
}

// both directions of the GGX prefilter of cubes' chains: x (cubes,6,T,C) -> y (cubes,6,T,C)
static int cube_prefilter(int32_t cubes, int32_t N, int32_t C, int32_t max_mip_level, int transpose, const float* x, float* y,
                          void* stream) {
    int64_t T;
    if (cubes < 0 || cubes > 10922) return fail("cube_prefilter: the number of cubes must lie in [0, 10922]");     // 6 * cubes <= 65535
    if (N < 1) return fail("cube_prefilter: N must be at least 1");
    if (C < 1 || C > dm2::cube_prefilter_max_channels()) return fail("cube_prefilter: the cube filter takes 1 to 262140 channels");
    dm2::mip_levels(N, N, max_mip_level, &T);
    if (6 * ((int64_t)N * N + T) > 0x7FFFFFFF) return fail("cube_prefilter: the texels of all levels of the cube must number below 2^31");
    if (cubes == 0 || T == 0) return 0;
    if (!x || !y) return fail("cube_prefilter: the cube filter's input and output chains must not be null");
    dm2::launch_cube_prefilter(cubes, N, C, max_mip_level, transpose, x, y, (hipStream_t)stream);
    DM2_HIP(hipGetLastError());
    return 0;
}

int dm2_cube_prefilter(int32_t cubes, int32_t N, int32_t C, int32_t max_mip_level, const float* x, float* y, void* stream) {
    return cube_prefilter(cubes, N, C, max_mip_level, 0, x, y, stream);
}

int dm2_cube_prefilter_backward(int32_t cubes, int32_t N, int32_t C, int32_t max_mip_level, const float* ybar, float* xbar,
                                void* stream) {
    return cube_prefilter(cubes, N, C, max_mip_level, 1, ybar, xbar, stream);
}

int dm2_texture_mipmaps(int32_t NB, int32_t Ht, int32_t Wt, int32_t C, int32_t max_mip_level, const float* tex, float* mip,
                        void* stream) {
    int64_t T;
    if (check_mip_sizes(NB, Ht, Wt, C, max_mip_level, &T)) return 1;
    if (NB == 0 || T == 0) return 0;
    if (!tex || !mip) return fail("texture_mipmaps: tex and mip must not be null");
    dm2::launch_texture_mipmaps(NB, Ht, Wt, C, max_mip_level, tex, mip, (hipStream_t)stream);
    DM2_HIP(hipGetLastError());
    return 0;
}

int dm2_texture_mipmaps_backward(int32_t NB, int32_t Ht, int32_t Wt, int32_t C, int32_t max_mip_level, const float* dL_dmip,
                                 float* dL_dtex, void* stream) {
    int64_t T;
    if (check_mip_sizes(NB, Ht, Wt, C, max_mip_level, &T)) return 1;
    if (NB == 0) return 0;
    if (!dL_dtex) return fail("texture_mipmaps_backward: dL_dtex must not be null");
    if (T == 0) {                                                        // no level depends on tex
        DM2_HIP(hipMemsetAsync(dL_dtex, 0, (size_t)NB * Ht * Wt * C * sizeof(float), (hipStream_t)stream));
        return 0;
    }
    if (!dL_dmip) return fail("texture_mipmaps_backward: dL_dmip must not be null");
    dm2::launch_texture_mipmaps_backward(NB, Ht, Wt, C, max_mip_level, dL_dmip, dL_dtex, (hipStream_t)stream);
    DM2_HIP(hipGetLastError());
    return 0;
}

static int check_texture_mip_sizes(int32_t B, int32_t H, int32_t W, int32_t L, int32_t Ht, int32_t Wt, int32_t C, int32_t boundary,
                                   int32_t max_mip_level, int64_t* T) {
    if (check_texture_sizes(B, H, W, L, Ht, Wt, C, DM2_TEX_FILTER_LINEAR, boundary)) return 1;
    return check_mip_sizes(B, Ht, Wt, C, max_mip_level, T);
}

int dm2_texture_mip(int32_t B, int32_t H, int32_t W, int32_t L, int32_t Ht, int32_t Wt, int32_t C, int32_t view_textures,
                    int32_t boundary, int32_t max_mip_level, const int32_t* render_layers, const float* uv, const float* uv_da,
                    const float* tex, const float* mip, float* out, void* stream) {
    int64_t T;
    if (check_texture_mip_sizes(B, H, W, L, Ht, Wt, C, boundary, max_mip_level, &T)) return 1;
    if ((int64_t)B * H * W * L == 0) return 0;
    if (!uv || !uv_da || !tex || !out) return fail("texture_mip: uv, uv_da, tex and out must not be null");
    if (T > 0 && !mip) return fail("texture_mip: mip must not be null");
    dm2::launch_texture_mip(B, H, W, L, Ht, Wt, C, view_textures, boundary, max_mip_level, render_layers, uv, uv_da, tex, mip, out,
                            (hipStream_t)stream);
    DM2_HIP(hipGetLastError());
    return 0;
}

int dm2_texture_mip_backward(int32_t B, int32_t H, int32_t W, int32_t L, int32_t Ht, int32_t Wt, int32_t C, int32_t view_textures,
                             int32_t boundary, int32_t max_mip_level, const int32_t* render_layers, const float* uv,
                             const float* uv_da, const float* tex, const float* mip, const float* dL_dout, float* dL_dtex,
                             float* dL_dmip, float* dL_duv, void* stream) {
    int64_t T;
    if (check_texture_mip_sizes(B, H, W, L, Ht, Wt, C, boundary, max_mip_level, &T)) return 1;
    if (T == 0) dL_dmip = nullptr;                                       // an empty chain: nothing to add into
    if ((int64_t)B * H * W * L == 0 || (!dL_dtex && !dL_dmip && !dL_duv)) return 0;
    if (!uv || !uv_da || !dL_dout) return fail("texture_mip_backward: uv, uv_da and dL_dout must not be null");
    if (dL_duv && (!tex || (T > 0 && !mip))) return fail("texture_mip_backward: tex and mip must not be null");
    dm2::launch_texture_mip_backward(B, H, W, L, Ht, Wt, C, view_textures, boundary, max_mip_level, render_layers, uv, uv_da, tex,
                                     mip, dL_dout, dL_dtex, dL_dmip, dL_duv, (hipStream_t)stream);
    DM2_HIP(hipGetLastError());
    return 0;
}

// a chain per face (*T: its texels), every level's texels in one 32-bit key space
static int check_texture_cube_mip_sizes(int32_t B, int32_t H, int32_t W, int32_t L, int32_t N, int32_t C, int32_t max_mip_level,
                                        int64_t* T) {
    if (check_texture_cube_sizes("texture_cube_mip", B, H, W, L, N, C, DM2_TEX_FILTER_LINEAR)) return 1;
    dm2::mip_levels(N, N, max_mip_level, T);
    if (6 * ((int64_t)N * N + *T) > 0x7FFFFFFF) return fail("texture_cube_mip: the texels of all levels of the cube must number below 2^31");
    return 0;
}

int dm2_texture_cube_mip(int32_t B, int32_t H, int32_t W, int32_t L, int32_t N, int32_t C, int32_t view_textures, int32_t max_mip_level,
                         const int32_t* render_layers, const float* dirs, const float* level, const float* tex, const float* mip,
                         float* out, void* stream) {
    int64_t T;
    if (check_texture_cube_mip_sizes(B, H, W, L, N, C, max_mip_level, &T)) return 1;
    if ((int64_t)B * H * W * L == 0) return 0;
    if (!dirs || !level || !tex || !out) return fail("texture_cube_mip: dirs, the level, tex and out must not be null");
    if (T > 0 && !mip) return fail("texture_cube_mip: mip must not be null");
    dm2::launch_texture_cube_mip(B, H, W, L, N, C, view_textures, max_mip_level, render_layers, dirs, level, tex, mip, out,
                                 (hipStream_t)stream);
    DM2_HIP(hipGetLastError());
    return 0;
}

int dm2_texture_cube_mip_backward(int32_t B, int32_t H, int32_t W, int32_t L, int32_t N, int32_t C, int32_t view_textures,
                                  int32_t max_mip_level, const int32_t* render_layers, const float* dirs, const float* level,
                                  const float* tex, const float* mip, const float* dL_dout, float* dL_dtex, float* dL_dmip,
                                  float* dL_drows, void* stream) {
    int64_t T;
    if (check_texture_cube_mip_sizes(B, H, W, L, N, C, max_mip_level, &T)) return 1;
    if (T == 0) dL_dmip = nullptr;                                       // an empty chain: nothing to add into
    if ((int64_t)B * H * W * L == 0 || (!dL_dtex && !dL_dmip && !dL_drows)) return 0;
    if (!dirs || !level || !dL_dout) return fail("texture_cube_mip_backward: dirs, the level and dL_dout must not be null");
    if (dL_drows && (!tex || (T > 0 && !mip))) return fail("texture_cube_mip_backward: tex and mip must not be null");
    if ((uintptr_t)dL_drows % 16) return fail("texture_cube_mip_backward: the cube's dL_drows rows must be 16-byte aligned");
    dm2::launch_texture_cube_mip_backward(B, H, W, L, N, C, view_textures, max_mip_level, render_layers, dirs, level, tex, mip,
                                          dL_dout, dL_dtex, dL_dmip, dL_drows, (hipStream_t)stream);
    DM2_HIP(hipGetLastError());
    return 0;
}

static int check_composite_sizes(int32_t B, int32_t H, int32_t W, int32_t L, int32_t C, int32_t F, int32_t alpha_mode) {
    if (B < 0 || H < 0 || W < 0 || L < 0 || F < 0) return fail("composite: negative size");
    if (C < 1 || C > (1 << 20)) return fail("composite: C must lie in [1, 2^20]");
    if (alpha_mode != DM2_COMPOSITE_ALPHA_PER_SLOT && alpha_mode != DM2_COMPOSITE_ALPHA_PER_FACE)
        return fail("composite: unknown alpha_mode");
    if (((int64_t)B * H * W + 255) / 256 > 0x7FFFFFFF || B > 65535 || ((int64_t)H + dm2::TILE - 1) / dm2::TILE > 65535)
        return fail("composite: too many pixels, rows or views");
    return 0;
}

int dm2_composite(int32_t B, int32_t H, int32_t W, int32_t L, int32_t C, int32_t F, int32_t alpha_mode, const float* values,
                  const float* alpha, const int32_t* render_layers, const float* background, float* out, float* out_acc,
                  float* out_final_T, int32_t* out_n_contrib, void* stream) {
    if (check_composite_sizes(B, H, W, L, C, F, alpha_mode)) return 1;
    if ((int64_t)B * H * W == 0) return 0;
    if (!out) return fail("composite: out must not be null");
    const int per_face = alpha_mode == DM2_COMPOSITE_ALPHA_PER_FACE;
    if (L > 0) {
        if (!values) return fail("composite: values must not be null");
        if (per_face && !render_layers) return fail("composite: a per-face alpha needs render_layers");
        if (!alpha && !(per_face && F == 0)) return fail("composite: alpha must not be null");
    }
    dm2::launch_composite(B, H, W, L, C, F, per_face, values, alpha, render_layers, background, out, out_acc, out_final_T,
                          out_n_contrib, (hipStream_t)stream);
    DM2_HIP(hipGetLastError());
    return 0;
}

int dm2_composite_backward(int32_t B, int32_t H, int32_t W, int32_t L, int32_t C, int32_t F, int32_t alpha_mode,
                           const float* values, const float* alpha, const int32_t* render_layers, const float* background,
                           const int32_t* n_contrib, const float* dL_dout, const float* dL_dacc, float* dL_dvalues,
                           float* dL_dalpha, void* stream) {
    if (check_composite_sizes(B, H, W, L, C, F, alpha_mode)) return 1;
    if ((int64_t)B * H * W == 0 || L == 0 || (!dL_dvalues && !dL_dalpha) || (!dL_dout && !dL_dacc)) return 0;
    const int per_face = alpha_mode == DM2_COMPOSITE_ALPHA_PER_FACE;
    if (!n_contrib) return fail("composite_backward: n_contrib must not be null");
    if (per_face && !render_layers) return fail("composite_backward: a per-face alpha needs render_layers");
    if (!alpha && !(per_face && F == 0)) return fail("composite_backward: alpha must not be null");
    if (dL_dalpha && dL_dout && !values) return fail("composite_backward: values must not be null");
    dm2::launch_composite_backward(B, H, W, L, C, F, per_face, values, alpha, render_layers, background, n_contrib, dL_dout,
                                   dL_dacc, dL_dvalues, dL_dalpha, (hipStream_t)stream);
    DM2_HIP(hipGetLastError());
    return 0;
}

static int check_coverage_sizes(int32_t B, int32_t H, int32_t W, int32_t L, int32_t P, int32_t F, float temperature) {
    if (B < 0 || H < 0 || W < 0 || L < 0 || P < 0 || F < 0) return fail("coverage: negative size");
    if (!(temperature >= 0.0f && temperature <= 1.0f)) return fail("coverage: temperature must be in the range [0, 1]");
    if (B > 65535 || ((int64_t)H + dm2::TILE - 1) / dm2::TILE > 65535) return fail("coverage: too many rows or views");
    return 0;
}

int dm2_coverage(int32_t B, int32_t H, int32_t W, int32_t L, int32_t P, int32_t F, float temperature, const dm2_window* win,
                 const int32_t* render_layers, const uint8_t* inside, const float* verts_image, const int32_t* faces,
                 float* out_cov, void* stream) {
    if (check_coverage_sizes(B, H, W, L, P, F, temperature)) return 1;
    if ((int64_t)B * H * W * L == 0) return 0;
    if (!render_layers || !out_cov) return fail("coverage: render_layers and out_cov must not be null");
    if (F > 0 && !faces) return fail("coverage: faces must not be null");
    if (F > 0 && P > 0 && !verts_image) return fail("coverage: verts_image must not be null");
    dm2::launch_coverage(B, H, W, L, P, F, temperature, win ? win->patch_min : nullptr, render_layers, inside, verts_image, faces, out_cov,
                         (hipStream_t)stream);
    DM2_HIP(hipGetLastError());
    return 0;
}

int dm2_coverage_backward(int32_t B, int32_t H, int32_t W, int32_t L, int32_t P, int32_t F, float temperature,
                          const dm2_window* win, const int32_t* render_layers, const float* verts_image,
                          const int32_t* faces, const float* dL_dcov, float* dL_dverts_image, void* stream) {
    if (check_coverage_sizes(B, H, W, L, P, F, temperature)) return 1;
    if ((int64_t)B * H * W * L == 0 || F == 0 || P == 0 || temperature == 0.0f || !dL_dcov || !dL_dverts_image) return 0;
    if (!render_layers || !faces || !verts_image) return fail("coverage_backward: render_layers, faces and verts_image must not be null");
    dm2::launch_coverage_backward(B, H, W, L, P, F, temperature, win ? win->patch_min : nullptr, render_layers, verts_image, faces, dL_dcov, dL_dverts_image,
                                  (hipStream_t)stream);
    DM2_HIP(hipGetLastError());
    return 0;
}

static int check_composite_desc(const dm2_layer_composite_desc* d) {
    if (!d) return fail("null descriptor");
    if (d->B < 0 || d->P < 0 || d->F < 0 || d->W < 0 || d->H < 0 || d->L < 0) return fail("negative size in descriptor");
    const int64_t gx = (d->W + dm2::TILE - 1) / dm2::TILE, gy = (d->H + dm2::TILE - 1) / dm2::TILE;
    if (gx > 0x7FFFFFFF || gy > 0xFFFF || d->B > 65535) return fail("image too large");
    const int64_t N = (int64_t)d->B * d->H * d->W;
    if (N == 0) return 0;
    if (!d->background) return fail("background must not be null");
    if (d->L > 0 && !d->render_layers) return fail("render_layers must not be null");
    if (d->F > 0 && (!d->faces || !d->verts || !d->verts_color || !d->faces_opacity || !d->faces_intense || !d->verts_ndc))
        return fail("the per-face / per-vertex inputs must not be null");
    if (d->flags & DM2_FLAG_ANALYTIC_RAYS) {
        if (!d->ray_cam) return fail("DM2_FLAG_ANALYTIC_RAYS needs ray_cam");
    } else if (!d->image_ray_o || !d->image_ray_d) {
        return fail("image_ray_o / image_ray_d must not be null");
    }
    return 0;
}

int dm2_layers_composite(const dm2_layer_composite_desc* d, const dm2_window* win, float* out_color, float* out_depth,
                         float* out_final_T, int32_t* out_n_contrib, float* out_face_weights, void* stream) {
    if (check_composite_desc(d)) return 1;
    dm2_window w;
    if (resolve_window(win, d->W, d->H, &w)) return 1;
    if ((int64_t)d->B * d->H * d->W == 0) return 0;
    if (!out_color || !out_depth || !out_n_contrib) return fail("out_color / out_depth / out_n_contrib must not be null");
    dm2::launch_layer_composite(*d, w, out_color, out_depth, out_final_T, out_n_contrib, out_face_weights, (hipStream_t)stream);
    DM2_HIP(hipGetLastError());
    return 0;
}

int dm2_layers_composite_backward(const dm2_layer_composite_desc* d, const dm2_window* win, const float* dL_dout_color,
                                  const float* dL_dout_depth, const float* dL_dout_alpha, const int32_t* n_contrib,
                                  float* dL_dverts_color, float* dL_dfaces_opacity, float* dL_dverts_ndc,
                                  float* dL_dfaces_intense, void* stream) {
    if (check_composite_desc(d)) return 1;
    dm2_window w;
    if (resolve_window(win, d->W, d->H, &w)) return 1;
    if ((int64_t)d->B * d->H * d->W == 0 || d->L == 0 || d->F == 0) return 0;       // nothing blends: all gradients stay zero
    if (!dL_dout_color || !dL_dout_depth || !n_contrib) return fail("dL_dout_color / dL_dout_depth / n_contrib must not be null");
    if (!dL_dverts_color || !dL_dfaces_opacity || !dL_dverts_ndc || !dL_dfaces_intense) return fail("gradient outputs must not be null");
    dm2::launch_layer_composite_backward(*d, w, dL_dout_color, dL_dout_depth, n_contrib, dL_dverts_color, dL_dfaces_opacity,
                                         dL_dverts_ndc, dL_dfaces_intense, dL_dout_alpha, (hipStream_t)stream);
    DM2_HIP(hipGetLastError());
    return 0;
}

static int check_prep_desc(const dm2_prep_desc* d) {
    if (!d) return fail("null descriptor");
    if (d->B < 0 || d->P < 0 || d->F < 0 || d->W < 0 || d->H < 0) return fail("negative size in descriptor");
    if (d->B > 65535) return fail("more than 65535 views per call");
    if (d->P > 0 && d->B > 0 && (!d->verts || !d->mv || !d->proj)) return fail("verts, mv and proj must not be null");
    if (d->F > 0 && !d->faces) return fail("faces must not be null");
    return 0;
}

int dm2_prepare_faces(const dm2_prep_desc* d, void* stream) {
    if (check_prep_desc(d)) return 1;
    const bool tables = d->aa_face_verts || d->aa_face_edges || d->aa_face_edges_iszero || d->aa_face_edges_recip ||
                        d->aa_face_edges_normal || d->aa_face_edges_normal_c;
    if (tables && d->F > 0 && d->B > 0 && !d->verts_image) return fail("the AA tables are built from verts_image: it must not be null");
    dm2::launch_prepare_faces(*d, (hipStream_t)stream);
    DM2_HIP(hipGetLastError());
    return 0;
}

int dm2_prepare_faces_backward(const dm2_prep_desc* d, const float* g_verts_ndc, const float* g_verts_image,
                               const float* g_aa_face_verts, float* image_grad_scratch, float* g_verts, void* stream) {
    if (check_prep_desc(d)) return 1;
    if (d->P > 0 && !g_verts) return fail("g_verts must not be null");
    return dm2_prepare_faces_backward_camera(d, g_verts_ndc, g_verts_image, g_aa_face_verts, image_grad_scratch, g_verts, nullptr,
                                             nullptr, nullptr, stream);
}

size_t dm2_prepare_faces_camera_scratch_bytes(int32_t B, int32_t P) { return dm2::prepare_camera_scratch_bytes(B, P); }

int dm2_prepare_faces_backward_camera(const dm2_prep_desc* d, const float* g_verts_ndc, const float* g_verts_image,
                                      const float* g_aa_face_verts, float* image_grad_scratch, float* g_verts, float* g_mv,
                                      float* g_proj, void* camera_scratch, void* stream) {
    if (check_prep_desc(d)) return 1;
    const bool camera = (g_mv || g_proj) && d->B > 0;
    if (g_aa_face_verts && d->F > 0 && d->B > 0 && d->P > 0 && (g_verts || camera) && !image_grad_scratch)
        return fail("image_grad_scratch must not be null");
    if (camera && dm2::prepare_camera_scratch_bytes(d->B, d->P) > 0 && !camera_scratch) return fail("camera_scratch must not be null");
    dm2::launch_prepare_faces_backward(*d, g_verts_ndc, g_verts_image, g_aa_face_verts, image_grad_scratch, g_verts, g_mv, g_proj,
                                       (double*)camera_scratch, (hipStream_t)stream);
    DM2_HIP(hipGetLastError());
    return 0;
}

static int check_exchange(int32_t B, int32_t P, int32_t F, int32_t N) {
    if (B < 0 || P < 0 || F < 0) return fail("negative size");
    if (N < 1 || N > dm2::exchange_max_ranks()) return fail("dm2_exchange_*: 1 <= N <= 64 ranks");
    return 0;
}

int dm2_exchange_mark(int32_t B, int32_t P, int32_t F, int32_t N, const int32_t* faces, const void* face_scratch, size_t face_bytes,
                      uint8_t* flags, uint32_t* counts, void* stream) {
    if (check_exchange(B, P, F, N)) return 1;
    if (!flags || !counts) return fail("dm2_exchange_mark: null output");
    const int64_t BF = (int64_t)B * F;
    const uint32_t* touched = nullptr;
    if (BF > 0 && P > 0) {
        if (!faces || !face_scratch) return fail("dm2_exchange_mark: null input");
        dm2::FaceState fs = dm2::FaceState::carve(const_cast<void*>(face_scratch), BF, 0, dm2::scan_temp_bytes(BF), false);
        touched = fs.tiles_touched;
        if ((size_t)((const char*)(touched + BF) - (const char*)face_scratch) > face_bytes) return fail("dm2_exchange_mark: face scratch too small");
    }
    DM2_HIP(dm2::launch_exchange_mark(B, P, F, N, faces, touched, flags, counts, (hipStream_t)stream));
    DM2_HIP(hipGetLastError());
    return 0;
}

int dm2_exchange_pack(int32_t B, int32_t P, int32_t F, int32_t N, const uint8_t* flags, const uint32_t* counts, uint32_t* cursors,
                      const float* dverts, const float* dverts_color, const float* dfaces_opacity, const float* dfaces_intense,
                      float* send, void* stream) {
    if (check_exchange(B, P, F, N)) return 1;
    if (!flags || !counts || !cursors) return fail("dm2_exchange_pack: null scratch");
    if (P > 0 && F > 0 && (!dverts || !dverts_color || !dfaces_opacity || !dfaces_intense)) return fail("dm2_exchange_pack: null gradient");
    DM2_HIP(dm2::launch_exchange_pack(B, P, F, N, flags, counts, cursors, dverts, dverts_color, dfaces_opacity, dfaces_intense, send, (hipStream_t)stream));
    DM2_HIP(hipGetLastError());
    return 0;
}

int dm2_exchange_unpack(int32_t B, int32_t P, int32_t F, int32_t N, int32_t rank, const float* recv, const uint32_t* recv_counts,
                        int64_t rows, float* slice_v, float* slice_f, void* stream) {
    if (check_exchange(B, P, F, N)) return 1;
    if (rank < 0 || rank >= N) return fail("dm2_exchange_unpack: rank out of range");
    if (!slice_v || !slice_f || !recv_counts || (rows > 0 && !recv)) return fail("dm2_exchange_unpack: null pointer");
    DM2_HIP(dm2::launch_exchange_unpack(B, P, F, N, rank, recv, recv_counts, rows, slice_v, slice_f, (hipStream_t)stream));
    DM2_HIP(hipGetLastError());
    return 0;
}

int dm2_debug_aa_overlap(int variant, int64_t n, const float* aa_face_verts, const float* aa_face_edges,
                         const uint8_t* aa_face_edges_iszero, const float* aa_face_edges_recip, const float* aa_face_edges_normal,
                         const float* aa_face_edges_normal_c, const float* pixmin, float* area, float* grad, int32_t* code,
                         void* stream) {
    if (variant < 0 || variant > 4) return fail("dm2_debug_aa_overlap: unknown variant");
    if (n < 0) return fail("dm2_debug_aa_overlap: negative count");
    if (n > 0 && (!aa_face_verts || !aa_face_edges || !aa_face_edges_iszero || !aa_face_edges_recip || !aa_face_edges_normal ||
                  !aa_face_edges_normal_c || !pixmin || !area || !grad || !code))
        return fail("dm2_debug_aa_overlap: null pointer");
    dm2::launch_debug_aa_overlap(variant, n, aa_face_verts, aa_face_edges, aa_face_edges_iszero, aa_face_edges_recip,
                                 aa_face_edges_normal, aa_face_edges_normal_c, pixmin, area, grad, code, (hipStream_t)stream);
    DM2_HIP(hipGetLastError());
    return 0;
}

int dm2_debug_fetch(int what, int64_t count, int64_t aux, int64_t num_rendered, const void* scratch, size_t scratch_bytes,
                    void* dst, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    void* base = const_cast<void*>(scratch);
    const void* src = nullptr; size_t bytes = 0;
    switch (what) {
        case 0: { auto s = dm2::ImageState::carve(base, count, aux); src = s.ranges; bytes = (size_t)aux * 8; break; }
        case 1: { auto s = dm2::BinningState::carve(base, num_rendered, dm2::sort_temp_bytes(num_rendered, aux)); src = s.face_list; bytes = (size_t)num_rendered * 4; break; }
        case 2: { auto s = dm2::ImageState::carve(base, count, aux); src = s.final_T; bytes = (size_t)count * 4; break; }
        case 3: { auto s = dm2::ImageState::carve(base, count, aux); src = s.final_prev_T; bytes = (size_t)count * 4; break; }
        case 4: { auto s = dm2::ImageState::carve(base, count, aux); src = s.n_contrib; bytes = (size_t)count * 4; break; }
        case 5: { auto s = dm2::LayerImageState::carve(base, count, aux); src = s.first_face; bytes = (size_t)count * 4; break; }
        case 6: { auto s = dm2::LayerImageState::carve(base, count, aux); src = s.first_tet; bytes = (size_t)count * 4; break; }
        case 7: { auto s = dm2::LayerImageState::carve(base, count, aux); src = s.ranges; bytes = (size_t)aux * 8; break; }
        case 8: { auto s = dm2::FaceState::carve(base, count, 0, dm2::scan_temp_bytes(count), false); src = s.tiles_touched; bytes = (size_t)count * 4; break; }
        case 9: { auto s = dm2::BinningState::carve(base, num_rendered, dm2::sort_temp_bytes(num_rendered, aux)); src = s.hit_valid; bytes = 4 * 4; break; }
        case 10: { auto s = dm2::BinningState::carve(base, num_rendered, dm2::sort_temp_bytes(num_rendered, aux)); src = s.hit_valid; bytes = 8 * 4; break; }
        default: return fail("dm2_debug_fetch: unknown item");
    }
    if (!scratch && bytes) return fail("dm2_debug_fetch: null scratch");
    if (bytes && (size_t)((const char*)src - (const char*)scratch) + bytes > scratch_bytes) return fail("dm2_debug_fetch: item lies beyond scratch_bytes");
    if (bytes) DM2_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, st));
    return 0;
}

}  // extern "C"
