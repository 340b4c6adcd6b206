// C-ABI implementation (include/sdrpp_gpu.h): context, streaming state, per-push planning and kernel launches.
// One context = one IQ stream on one GPU; everything is enqueued on one HIP stream so a push is a fixed sequence of
// launches whose sizes are computed on the host from integer state (decimation offsets, polyphase phase, frame position).
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <algorithm>
#include <chrono>
#include <atomic>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <deque>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/sdrpp_gpu.h"
#include "fft_kernels.h"
#include "host_design.h"
#include "vfo_kernels.h"
#include "pipe_kernels.h"
#include "tick_kernels.h"

using namespace sdrpp_k;

#include "host_ctx.h"
#include "host_util.h"
#include "plan_fft.h"
#include "plan_vfo.h"
#include "plan_pre.h"
#include "plan_push.h"
#include "tick_host.h"
#include "vfo_ctl.h"

// =====================================================================================================================
// C ABI
// =====================================================================================================================
// HIP's current device is a per-THREAD setting: a host that owns several contexts on several GPUs (StreamBank, one worker thread
// per IQFrontEnd) calls into a context from threads whose current device is some other GPU.  Every entry point that takes a context
// therefore makes the context's device current for the duration of the call (allocations, launches, copies, symbol accesses all
// follow the current device) and restores the caller's on return.
struct DeviceScope {
    int prev = -1;
    explicit DeviceScope(const sdrpp_ctx* c) {
        if (!c) { return; }
        int cur = -1;
        if (hipGetDevice(&cur) == hipSuccess && cur != c->device) {
            prev = cur;
            (void)hipSetDevice(c->device);
        }
    }
    ~DeviceScope() {
        if (prev >= 0) { (void)hipSetDevice(prev); }
    }
    DeviceScope(const DeviceScope&) = delete;
    DeviceScope& operator=(const DeviceScope&) = delete;
};
// every call that observes results or changes the configuration first processes what deferred pushes have staged
#define FLUSH_PENDING(c)                          \
    do {                                          \
        int frc_ = flush_pending(c);              \
        if (frc_) { return frc_; }                \
    } while (0)
// ... and every call that takes a VFO id then looks it up (vfo_lookup has set the message)
#define LOOKUP_VFO(v, c, id)    \
    Vfo* v = vfo_lookup(c, id); \
    if (!v) { return SDRPP_ERR_NOT_FOUND; }

extern "C" {

int flush_pending(sdrpp_ctx* c);  // deferred pushes -> one pass (defined with the data path below; internal, not part of the ABI header)
int flush_pending_opt(sdrpp_ctx* c, int drain);  // drain = 0: a call that only reports what the HOST knows (counts) leaves the tick queue of the pipelined mode alone

const char* sdrpp_strerror(int code) {
    switch (code) {
    case SDRPP_OK: return "ok";
    case SDRPP_ERR_NO_DEVICE: return "no usable HIP device (this library has no CPU fallback)";
    case SDRPP_ERR_INVALID: return "invalid argument or call sequence";
    case SDRPP_ERR_NOMEM: return "device memory allocation failed";
    case SDRPP_ERR_HIP: return "HIP runtime error";
    case SDRPP_ERR_UNSUPPORTED: return "unsupported parameter";
    case SDRPP_ERR_NOT_FOUND: return "no such VFO";
    default: return "unknown error";
    }
}

int sdrpp_abi_version(int* sizeof_vfo_desc) {  // 2: sdrpp_vfo_desc carries nco_mode (round 3); sdrpp_pipeline_stats
    if (sizeof_vfo_desc) { *sizeof_vfo_desc = (int)sizeof(sdrpp_vfo_desc); }
    return SDRPP_ABI_VERSION;
}

const char* sdrpp_kernel_family_name(int family) { return (family >= 0 && family < SDRPP_NUM_KERNEL_FAMILIES) ? kFamilyNames[family] : "?"; }

int sdrpp_device_count(void) {
    int n = 0;
    return (hipGetDeviceCount(&n) == hipSuccess) ? n : 0;
}

int sdrpp_create(int device, int64_t max_push, sdrpp_ctx** out) {
    if (!out || max_push <= 0 || max_push > ((int64_t)1 << 28)) { return SDRPP_ERR_INVALID; }
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) { return SDRPP_ERR_NO_DEVICE; }
    if (hipSetDevice(device) != hipSuccess) { return SDRPP_ERR_NO_DEVICE; }
    sdrpp_ctx* c = new sdrpp_ctx;
    c->device = device;
    c->max_push = max_push;
    if (const char* tf = getenv("SDRPP_GPU_TEST_FAIL_ARENA")) {
        long a = 0;
        int b = 0;
        if (sscanf(tf, "%ld:%d", &a, &b) == 2) {
            c->test_fail_pass = a;
            c->test_fail_alloc = b;
        }
    }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess) {
        char b[600];
        snprintf(b, sizeof(b), "%s (%s, %d CUs)", prop.name, prop.gcnArchName, prop.multiProcessorCount);
        c->devinfo = b;
        c->num_cus = std::max(1, prop.multiProcessorCount);
        // the long-first-stage role with four tile engines asks for up to 80 KB of dynamic LDS per workgroup (two workgroups per CU): above the
        // 64 KB a launch gets without asking
        // (tick_kernel<0> as well: a long first stage whose window does NOT fit the register prefetch — nsamp > 64 * SDRPP_FCL_PF, a custom plan with
        // a very long /64 stage — goes out as role TR_FCL_0 in the SET = 0 build with the same four-engine LDS request)
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&tick_kernel<1>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 / 2);
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&tick_kernel<0>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 / 2);
        (void)hipGetLastError();
    }
    if (hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking) != hipSuccess) {
        delete c;
        return SDRPP_ERR_NO_DEVICE;
    }
    c->stream = c->own_stream;
    c->launch_stream = c->stream;
    {   // the FFT branch's stream gets the LOWEST queue priority: it is the filler behind the VFO bank, whose launches form the critical
        // path (measured on the headline step: 0.686-0.693 ms against 0.704-0.706 at equal priority and 0.699-0.701 with the FFT favoured)
        int lo = 0, hi = 0;
        (void)hipDeviceGetStreamPriorityRange(&lo, &hi);  // lo = least (numerically largest), hi = greatest
        if (hipStreamCreateWithPriority(&c->fft_stream, hipStreamNonBlocking, lo) != hipSuccess) { c->fft_stream = nullptr; }
    }
    if ((!c->fft_stream && hipStreamCreateWithFlags(&c->fft_stream, hipStreamNonBlocking) != hipSuccess) || hipEventCreate(&c->ev_fork) != hipSuccess ||
        hipEventCreate(&c->ev_join) != hipSuccess) {
        sdrpp_destroy(c);
        return SDRPP_ERR_NO_DEVICE;
    }
    for (int i = 0; i < kArenaSlots; i++) {
        if (hipHostMalloc((void**)&c->arena_host[i], kArenaBytes, hipHostMallocMapped) != hipSuccess ||
            hipHostGetDevicePointer((void**)&c->arena_host_dev[i], c->arena_host[i], 0) != hipSuccess || hipEventCreate(&c->arena_ev[i]) != hipSuccess) {
            sdrpp_destroy(c);
            return SDRPP_ERR_NOMEM;
        }
    }
    if (hipStreamCreateWithFlags(&c->side_stream, hipStreamNonBlocking) != hipSuccess) {
        sdrpp_destroy(c);
        return SDRPP_ERR_NO_DEVICE;
    }
    if (hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking) != hipSuccess || hipEventCreate(&c->ev_copy) != hipSuccess ||
        hipEventCreate(&c->land_ev[0]) != hipSuccess || hipEventCreate(&c->land_ev[1]) != hipSuccess) {
        sdrpp_destroy(c);
        return SDRPP_ERR_NO_DEVICE;
    }
    for (int i = 0; i < kArenaSlots; i++) {
        if (dev_alloc(c, &c->arena_dev_slot[i], kArenaBytes) != SDRPP_OK) {
            sdrpp_destroy(c);
            return SDRPP_ERR_NOMEM;
        }
    }
    c->arena_dev = c->arena_dev_slot[0];
    if (dev_alloc(c, &c->iq_land[0], (size_t)max_push * 2 + 32) != SDRPP_OK) {
        sdrpp_destroy(c);
        return SDRPP_ERR_NOMEM;
    }
    // completion flag and counter of the pipelined mode (sdrpp_set_pipelined)
    if (dev_alloc(c, &c->d_tick_counter, 4) != SDRPP_OK || dev_alloc(c, &c->empty_tab, 1) != SDRPP_OK ||
        hipMemset(c->d_tick_counter, 0, 16) != hipSuccess || hipMemset(c->empty_tab, 0, sizeof(TickTable)) != hipSuccess ||
        hipHostMalloc((void**)&c->h_tick_flag, 64, hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess ||
        hipHostGetDevicePointer((void**)&c->hd_tick_flag, c->h_tick_flag, 0) != hipSuccess) {
        sdrpp_destroy(c);
        return SDRPP_ERR_NOMEM;
    }
    *c->h_tick_flag = 0;
    c->h_tick_flag[8] = 0;  // flag waits that gave up (PipeJob::timeouts)
    *out = c;
    return SDRPP_OK;
}

// ---- WaterFall display state ----------------------------------------------------------------------------------
static void wf_free(sdrpp_ctx* c) {
    dev_free(c->wf.d_ring);
    dev_free(c->wf.d_latest);
    dev_free(c->wf.d_smooth);
    dev_free(c->wf.d_hold);
    c->wf = sdrpp_ctx::Wf{};
}

int sdrpp_wf_configure(sdrpp_ctx* c, int height) {
    DeviceScope dev_scope_(c);
    if (!c || height < 0) { return SDRPP_ERR_INVALID; }
    FLUSH_PENDING(c);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (c->fft_stream) { HIPCHK(c, hipStreamSynchronize(c->fft_stream)); }
    wf_free(c);
    if (height == 0) { return SDRPP_OK; }
    if (!c->fft_on) { return fail(c, SDRPP_ERR_INVALID, "configure the FFT first (sdrpp_fft_configure)"); }
    int rc = dev_alloc(c, &c->wf.d_ring, (size_t)height * c->fft_size);
    if (rc) { return rc; }
    HIPCHK(c, hipMemset(c->wf.d_ring, 0, (size_t)height * c->fft_size * sizeof(float)));
    c->wf.height = height;
    return SDRPP_OK;
}

int sdrpp_wf_set_smoothing(sdrpp_ctx* c, int enabled, float speed) {
    DeviceScope dev_scope_(c);
    if (!c) { return SDRPP_ERR_INVALID; }
    FLUSH_PENDING(c);
    if (c->wf.height <= 0) { return fail(c, SDRPP_ERR_INVALID, "no waterfall history configured (sdrpp_wf_configure)"); }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (c->fft_stream) { HIPCHK(c, hipStreamSynchronize(c->fft_stream)); }
    int rc = wf_ensure_trace(c);
    if (rc) { return rc; }
    sdrpp_ctx::Wf& W = c->wf;
    dev_free(W.d_smooth);  // setFFTSmoothing (waterfall.cpp:1166-1188): the buffer is re-created as a copy of latestFFT
    if (enabled && W.width > 0) {
        rc = dev_alloc(c, &W.d_smooth, (size_t)W.width);
        if (rc) { return rc; }
        HIPCHK(c, hipMemcpy(W.d_smooth, W.d_latest, (size_t)W.width * sizeof(float), hipMemcpyDeviceToDevice));
    }
    W.alpha = speed;  // setFFTSmoothingSpeed (:1190-1194)
    W.beta = 1.0f - speed;
    return SDRPP_OK;
}

int sdrpp_wf_set_hold(sdrpp_ctx* c, int enabled, float speed) {
    DeviceScope dev_scope_(c);
    if (!c) { return SDRPP_ERR_INVALID; }
    FLUSH_PENDING(c);
    if (c->wf.height <= 0) { return fail(c, SDRPP_ERR_INVALID, "no waterfall history configured (sdrpp_wf_configure)"); }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (c->fft_stream) { HIPCHK(c, hipStreamSynchronize(c->fft_stream)); }
    int rc = wf_ensure_trace(c);
    if (rc) { return rc; }
    sdrpp_ctx::Wf& W = c->wf;
    W.hold_on = enabled != 0;
    if (W.hold_on && W.width > 0) {  // setFFTHold (:1153-1160)
        std::vector<float> init((size_t)W.width, -1000.0f);
        HIPCHK(c, hipMemcpy(W.d_hold, init.data(), init.size() * sizeof(float), hipMemcpyHostToDevice));
    }
    W.hold_speed = speed;
    return SDRPP_OK;
}

int sdrpp_wf_latest(sdrpp_ctx* c, float* latest, float* hold) {
    DeviceScope dev_scope_(c);
    if (!c) { return SDRPP_ERR_INVALID; }
    FLUSH_PENDING(c);
    sdrpp_ctx::Wf& W = c->wf;
    if (W.height <= 0 || W.width <= 0 || !W.d_latest) { return fail(c, SDRPP_ERR_INVALID, "no waterfall trace yet"); }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (latest) { HIPCHK(c, hipMemcpy(latest, W.d_latest, (size_t)W.width * sizeof(float), hipMemcpyDeviceToHost)); }
    if (hold) { HIPCHK(c, hipMemcpy(hold, W.d_hold, (size_t)W.width * sizeof(float), hipMemcpyDeviceToHost)); }
    return W.width;
}

// updateWaterfallFb (waterfall.cpp:600-631): every stored line re-zoomed with a NEW view, newest first
int sdrpp_wf_raster(sdrpp_ctx* c, int draw_start, int draw_size, int data_width, float wf_min, float wf_max, int32_t* dst_host, int* n_lines) {
    DeviceScope dev_scope_(c);
    if (!c || !dst_host || data_width <= 0) { return SDRPP_ERR_INVALID; }
    FLUSH_PENDING(c);
    sdrpp_ctx::Wf& W = c->wf;
    if (W.height <= 0) { return fail(c, SDRPP_ERR_INVALID, "no waterfall history configured (sdrpp_wf_configure)"); }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (c->fft_stream) { HIPCHK(c, hipStreamSynchronize(c->fft_stream)); }
    const int count = std::min(W.lines, W.height);
    std::vector<int32_t> zs, zc;
    sdrpp_host::zoomTable(draw_start, draw_size, c->fft_size, data_width, zs, zc);
    int32_t *d_zs = nullptr, *d_zc = nullptr, *d_idx = nullptr;
    float* d_zm = nullptr;
    int rc = upload(c, &d_zs, zs.data(), zs.size());
    if (!rc) { rc = upload(c, &d_zc, zc.data(), zc.size()); }
    if (!rc) { rc = dev_alloc(c, &d_zm, (size_t)std::max(count, 1) * data_width); }
    if (!rc) { rc = dev_alloc(c, &d_idx, (size_t)std::max(count, 1) * data_width); }
    if (!rc && count > 0) {
        // display row i = ring slot (i + cur) mod H: two contiguous runs of slots
        const int first = std::min(count, W.height - W.cur);
        launch_zoom(c->stream, W.d_ring + (size_t)W.cur * c->fft_size, first, c->fft_size, draw_size, data_width, d_zs, d_zc, wf_min, wf_max, d_zm, d_idx);
        if (count > first) {
            launch_zoom(c->stream, W.d_ring, count - first, c->fft_size, draw_size, data_width, d_zs, d_zc, wf_min, wf_max, d_zm + (size_t)first * data_width, d_idx + (size_t)first * data_width);
        }
        hipError_t e = hipStreamSynchronize(c->stream);
        if (e == hipSuccess) { e = hipMemcpy(dst_host, d_idx, (size_t)count * data_width * sizeof(int32_t), hipMemcpyDeviceToHost); }
        if (e != hipSuccess) { rc = fail(c, SDRPP_ERR_HIP, "waterfall raster failed: %s", hipGetErrorString(e)); }
    }
    dev_free(d_zs);
    dev_free(d_zc);
    dev_free(d_zm);
    dev_free(d_idx);
    if (rc) { return rc; }
    for (size_t i = (size_t)count * data_width; i < (size_t)W.height * data_width; i++) { dst_host[i] = -1; }  // (uint32_t)255 << 24 in the reference
    if (n_lines) { *n_lines = count; }
    return SDRPP_OK;
}

static void preproc_free(sdrpp_ctx* c) {
    sdrpp_ctx::Pre& P = c->pre;
    rate_free(P.rate);
    P.raw.data = nullptr;  // the caller's buffer, never owned
    stream_free(P.raw);
    for (auto& s : P.st) { stream_free(s); }
    stream_free(P.out);
    dev_free(P.d_off);
    dev_free(P.d_seg);
    P = sdrpp_ctx::Pre{};
}

int sdrpp_destroy(sdrpp_ctx* c) {
    DeviceScope dev_scope_(c);
    if (!c) { return SDRPP_OK; }
    if (c->stream) { (void)hipStreamSynchronize(c->stream); }
    g_hostprof.report();
#ifdef SDRPP_TICK_TRACE
    if (const char* path = getenv("SDRPP_TICK_TRACE_FILE")) {
        unsigned n = 0;
        if (hipMemcpyFromSymbol(&n, HIP_SYMBOL(sdrpp_k::g_tick_trace_n), sizeof(n)) == hipSuccess && n > 0) {
            n = std::min<unsigned>(n, SDRPP_TICK_TRACE_CAP);
            std::vector<sdrpp_k::TickTraceRec> recs(n);
            if (hipMemcpyFromSymbol(recs.data(), HIP_SYMBOL(sdrpp_k::g_tick_trace), (size_t)n * sizeof(sdrpp_k::TickTraceRec)) == hipSuccess) {
                if (FILE* f = fopen(path, "ab")) {
                    fwrite(recs.data(), sizeof(sdrpp_k::TickTraceRec), n, f);
                    fclose(f);
                }
            }
            const unsigned zero = 0;
            (void)hipMemcpyToSymbol(HIP_SYMBOL(sdrpp_k::g_tick_trace_n), &zero, sizeof(zero));
        }
    }
#endif
#ifdef SDRPP_TOEP_PROF
    {
        unsigned long long h[4][8];
        if (hipMemcpyFromSymbol(h, HIP_SYMBOL(sdrpp_k::g_toep_prof), sizeof(h)) == hipSuccess) {
            const char* names[4] = { "decimator", "resampler", "channel filter", "discriminator+audio" };
            for (int k = 0; k < 4; k++) {
                if (!h[k][5]) { continue; }
                const double r = (double)h[k][5];
                fprintf(stderr, "[sdrpp toep prof] %-20s rounds %llu, cycles per round: matrix %.0f | wait loads + regs->LDS %.0f | issue loads %.0f | discriminate %.0f | issue stores %.0f ; wavefront lifetime %.0f cycles, %.2f rounds per wavefront\n",
                        names[k], h[k][5], h[k][0] / r, h[k][1] / r, h[k][2] / r, h[k][3] / r, h[k][4] / r, (double)h[k][6] / (double)h[k][7], r / (double)h[k][7]);
            }
            unsigned long long z[4][8] = {};
            (void)hipMemcpyToSymbol(HIP_SYMBOL(sdrpp_k::g_toep_prof), z, sizeof(z));
        }
        if (hipMemcpyFromSymbol(h, HIP_SYMBOL(sdrpp_k::g_pipe_prof), sizeof(h)) == hipSuccess) {
            const char* names[4] = { "decimator", "resampler", "channel filter", "discriminator+audio" };
            for (int k = 0; k < 4; k++) {
                if (!h[k][5]) { continue; }
                const double r = (double)h[k][5];
                fprintf(stderr, "[sdrpp pipe prof] %-20s tiles %llu, cycles per tile: wait input %.0f | matrix %.0f | release / stage next %.0f | epilogue + wait space %.0f | write + publish %.0f ; wavefront lifetime %.0f cycles, %.2f tiles per wavefront\n",
                        names[k], h[k][5], h[k][0] / r, h[k][1] / r, h[k][2] / r, h[k][3] / r, h[k][4] / r, (double)h[k][6] / (double)h[k][7], r / (double)h[k][7]);
            }
            unsigned long long z[4][8] = {};
            (void)hipMemcpyToSymbol(HIP_SYMBOL(sdrpp_k::g_pipe_prof), z, sizeof(z));
            unsigned long long ck[4] = { 0, 0, 0, 0 };
            if (hipMemcpyFromSymbol(ck, HIP_SYMBOL(sdrpp_k::g_pipe_clock), sizeof(ck)) == hipSuccess && ck[1]) {
                fprintf(stderr, "[sdrpp pipe prof] shader clock while the pipelined kernel ran: %.0f MHz (s_memtime cycles per 100 MHz s_memrealtime tick); wavefront lifetime min %llu max %llu cycles (all launches)\n",
                        100.0 * (double)ck[0] / (double)ck[1], ck[2], ck[3]);
            }
        }
    }
#endif
    preproc_free(c);
    wf_free(c);
    dev_free(c->meters.d_offs);
    dev_free(c->meters.d_out);
    dev_free(c->d_pack);
    dev_free(c->d_gather);
    dev_free(c->d_gather_jobs);
    for (auto& kv : c->vfos) { vfo_free(*kv.second); }
    for (auto& kv : c->rds_banks) { dev_free(kv.second.d_bank); }
    c->rds_banks.clear();
    for (auto& kv : c->sym_banks) { dev_free(kv.second.d_bank); }
    for (auto& kv : c->frame_tabs) { dev_free(kv.second.d_table); }
    c->frame_tabs.clear();
    for (auto& kv : c->rdsd_banks) {
        dev_free(kv.second.d_taps);
        dev_free(kv.second.d_bank);
    }
    c->rdsd_banks.clear();
    for (auto& kv : c->qpsk_banks) {
        dev_free(kv.second.d_taps);
        dev_free(kv.second.d_bank);
    }
    c->qpsk_banks.clear();
    c->sym_banks.clear();
    c->vfos.clear();
    for (auto& e : c->s1_tap_cache) { (void)hipFree(e.second); }
    for (auto& e : c->fmif_tabs) { (void)hipFree(e.second); }
    for (auto& p : c->tpairs) { (void)hipEventDestroy(p.a); (void)hipEventDestroy(p.b); }
    for (auto e : c->ev_pool) { (void)hipEventDestroy(e); }
    for (int i = 0; i < kArenaSlots; i++) {
        if (c->arena_host[i]) { (void)hipHostFree(c->arena_host[i]); }
        if (c->arena_ev[i]) { (void)hipEventDestroy(c->arena_ev[i]); }
    }
    for (int i = 0; i < kArenaSlots; i++) { dev_free(c->arena_dev_slot[i]); }
    c->arena_dev = nullptr;
    dev_free(c->d_tick_counter);
    dev_free(c->empty_tab);
    if (c->h_tick_flag) { (void)hipHostFree(c->h_tick_flag); }
    for (int i = 0; i < 3; i++) { dev_free(c->tick_land[i]); }
    for (int i = 0; i < kStageSlots; i++) {
        if (c->stage_host[i]) { (void)hipHostFree(c->stage_host[i]); }
    }
    if (c->bank_plan && c->bank_plan_free) { c->bank_plan_free(c->bank_plan); }
    c->bank_plan = nullptr;
    for (int i = 0; i < sdrpp_ctx::kTickEvents; i++) {
        if (c->tick_ev[i]) { (void)hipEventDestroy(c->tick_ev[i]); }
        if (c->tick_ev_start[i]) { (void)hipEventDestroy(c->tick_ev_start[i]); }
    }
    if (c->res_ring) { (void)hipHostFree(c->res_ring); }
    for (auto& q : c->res_retired) { (void)hipHostFree(q.ring); }
    c->res_retired.clear();
    fft_ring_drop(c);
    for (int i = 0; i < 2; i++) {
        dev_free(c->iq_land[i]);
        dev_free(c->iq_land16[i]);
        if (c->land_ev[i]) { (void)hipEventDestroy(c->land_ev[i]); }
    }
    dev_free(c->d_u8_tab);
    if (c->ev_copy) { (void)hipEventDestroy(c->ev_copy); }
    if (c->copy_stream) { (void)hipStreamDestroy(c->copy_stream); }
    if (c->side_stream) { (void)hipStreamDestroy(c->side_stream); }
    dev_free(c->iq_hist[0]);
    dev_free(c->iq_hist[1]);
    dev_free(c->d_window);
    dev_free(c->d_tw1);
    dev_free(c->d_tw2);
    dev_free(c->d_twn);
    dev_free(c->d_scratch);
    dev_free(c->d_lines);
    dev_free(c->d_lines_grp);
    dev_free(c->d_zstart);
    dev_free(c->d_zcount);
    dev_free(c->d_zoomed);
    dev_free(c->d_index);
    if (c->ev_fork) { (void)hipEventDestroy(c->ev_fork); }
    if (c->ev_join) { (void)hipEventDestroy(c->ev_join); }
    if (c->fft_stream) { (void)hipStreamDestroy(c->fft_stream); }
    if (c->own_stream) { (void)hipStreamDestroy(c->own_stream); }
    delete c;
    return SDRPP_OK;
}

const char* sdrpp_last_error(const sdrpp_ctx* c) { return c ? c->err.c_str() : "null context"; }

int sdrpp_set_stream(sdrpp_ctx* c, void* s) {
    DeviceScope dev_scope_(c);
    if (!c) { return SDRPP_ERR_INVALID; }
    FLUSH_PENDING(c);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->stream = s ? (hipStream_t)s : c->own_stream;
    c->launch_stream = c->stream;
    return SDRPP_OK;
}

int sdrpp_sync(sdrpp_ctx* c) {
    DeviceScope dev_scope_(c);
    if (!c) { return SDRPP_ERR_INVALID; }
    FLUSH_PENDING(c);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (int rc = pipe_timeouts_check(c)) { return rc; }
    return SDRPP_OK;
}

int sdrpp_device_info(sdrpp_ctx* c, char* buf, int buflen) {
    DeviceScope dev_scope_(c);
    if (!c || !buf || buflen <= 0) { return SDRPP_ERR_INVALID; }
    snprintf(buf, (size_t)buflen, "%s", c->devinfo.c_str());
    return SDRPP_OK;
}

// ---- FFT ---------------------------------------------------------------------------------------------------------------------
int sdrpp_fft_configure(sdrpp_ctx* c, int fft_size, int nz, int skip, const float* window) {
    DeviceScope dev_scope_(c);
    if (!c || !window) { return SDRPP_ERR_INVALID; }
    FLUSH_PENDING(c);
    if (!is_pow2(fft_size) || fft_size < 1024 || fft_size > (1 << 20)) { return fail(c, SDRPP_ERR_UNSUPPORTED, "fft_size %d: need a power of two in [1024, 1048576]", fft_size); }
    if (nz <= 0 || nz > fft_size || skip < 0) { return fail(c, SDRPP_ERR_INVALID, "bad framing nz=%d skip=%d", nz, skip); }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (c->fft_stream) { HIPCHK(c, hipStreamSynchronize(c->fft_stream)); }
    if (c->wf.height > 0 && fft_size != c->fft_size) { wf_free(c); }  // the line history holds lines of the old size (setRawFFTSize reallocates rawFFTs)
    c->fft_on = false;
    const int m = ilog2(fft_size);
    int rc = upload(c, &c->d_window, window, (size_t)nz);
    if (rc) { return rc; }
    auto half_table = [](int L) {
        std::vector<float2> t((size_t)std::max(L / 2, 1));
        for (int e = 0; e < L / 2; e++) { sdrpp_host::twiddle(e, L, &t[(size_t)e].x, &t[(size_t)e].y); }
        return t;
    };
    fft_ring_drop(c);
    dev_free(c->d_tw2);
    dev_free(c->d_twn);
    dev_free(c->d_scratch);
    if (m <= 12) {
        auto t = half_table(fft_size);
        rc = upload(c, &c->d_tw1, t.data(), t.size());
        if (rc) { return rc; }
    }
    else {
        int lg1, lg2;
        fft_split(m, &lg1, &lg2);
        const int N1 = 1 << lg1, N2 = 1 << lg2;
        auto t1 = half_table(N1);
        auto t2 = half_table(N2);
        rc = upload(c, &c->d_tw1, t1.data(), t1.size());
        if (rc) { return rc; }
        rc = upload(c, &c->d_tw2, t2.data(), t2.size());
        if (rc) { return rc; }
        std::vector<float2> full((size_t)fft_size);
        for (int e = 0; e < fft_size; e++) { sdrpp_host::twiddle(e, fft_size, &full[(size_t)e].x, &full[(size_t)e].y); }
        std::vector<float2> tn((size_t)fft_size);
        for (int k1 = 0; k1 < N1; k1++) {
            for (int n2 = 0; n2 < N2; n2++) { tn[(size_t)k1 * N2 + n2] = full[(size_t)k1 * n2]; }
        }
        rc = upload(c, &c->d_twn, tn.data(), tn.size());
        if (rc) { return rc; }
        const size_t per_chunk = std::max<size_t>(1, kScratchBytes / ((size_t)fft_size * sizeof(float2)));
        rc = dev_alloc(c, &c->d_scratch, per_chunk * (size_t)fft_size);
        if (rc) { return rc; }
    }
    const size_t lines = (size_t)(c->max_push / ((int64_t)nz + skip)) + 2;
    dev_free(c->d_lines);
    rc = dev_alloc(c, &c->d_lines, lines * (size_t)fft_size);
    if (rc) { return rc; }
    dev_free(c->d_lines_grp);
    c->d_lines_grp = nullptr;
    c->zoom_grp = (m > 16) ? kZoomGrpLong : ((m > 12) ? pass2_rows(m - m / 2) : 0);
    if (c->zoom_grp) {
        rc = dev_alloc(c, &c->d_lines_grp, lines * (size_t)(fft_size / c->zoom_grp));
        if (rc) { return rc; }
    }
    c->lines_cap = lines;
    c->fft_size = fft_size;
    c->fft_lg = m;
    c->nz = nz;
    c->skip = skip;
    c->fft_pos = 0;
    c->fft_next = 0;
    c->n_lines = 0;
    c->fft_on = true;
    rc = meters_rebuild(c);  // the table of signal meters is kept as frequencies: its bin offsets follow the size
    if (rc) { return rc; }
    if (c->data_width > 0) { return sdrpp_fft_set_view(c, c->view_start, c->view_size, c->data_width, c->wf_min, c->wf_max); }
    return SDRPP_OK;
}

int sdrpp_fft_disable(sdrpp_ctx* c) {
    DeviceScope dev_scope_(c);
    if (!c) { return SDRPP_ERR_INVALID; }
    FLUSH_PENDING(c);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->fft_on = false;
    c->n_lines = 0;
    return SDRPP_OK;
}

int sdrpp_fft_set_view(sdrpp_ctx* c, int start, int size, int data_width, float wf_min, float wf_max) {
    DeviceScope dev_scope_(c);
    if (!c || data_width < 0) { return SDRPP_ERR_INVALID; }
    FLUSH_PENDING(c);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->view_start = start;
    c->view_size = size;
    c->data_width = data_width;
    c->wf_min = wf_min;
    c->wf_max = wf_max;
    c->zoom_cap = 0;
    fft_ring_drop(c);
    dev_free(c->d_zoomed);
    dev_free(c->d_index);
    if (data_width == 0 || c->fft_size == 0) { return SDRPP_OK; }
    std::vector<int32_t> zs, zc;
    sdrpp_host::zoomTable(start, size, c->fft_size, data_width, zs, zc);
    int rc = upload(c, &c->d_zstart, zs.data(), zs.size());
    if (rc) { return rc; }
    rc = upload(c, &c->d_zcount, zc.data(), zc.size());
    if (rc) { return rc; }
    c->h_zstart = zs;
    c->h_zcount = zc;
    c->zoom_tp_cache = 0;
    return ensure_zoom(c, c->lines_cap);
}

int sdrpp_fft_lines(sdrpp_ctx* c) {
    DeviceScope dev_scope_(c);
    if (!c) { return SDRPP_ERR_INVALID; }
    {
        int frc = flush_pending_opt(c, 0);
        if (frc) { return frc; }
    }
    return c->n_lines;
}

int sdrpp_fft_read(sdrpp_ctx* c, int first, int n, float* raw, float* zoomed, int32_t* index) {
    DeviceScope dev_scope_(c);
    if (!c || first < 0 || n < 0) { return SDRPP_ERR_INVALID; }
    FLUSH_PENDING(c);
    if (first >= c->n_lines) { return 0; }
    n = std::min(n, c->n_lines - first);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (raw) { HIPCHK(c, hipMemcpy(raw, c->d_lines + (size_t)first * c->fft_size, (size_t)n * c->fft_size * sizeof(float), hipMemcpyDeviceToHost)); }
    if (c->data_width > 0) {
        if (zoomed) { HIPCHK(c, hipMemcpy(zoomed, c->d_zoomed + (size_t)first * c->data_width, (size_t)n * c->data_width * sizeof(float), hipMemcpyDeviceToHost)); }
        if (index) { HIPCHK(c, hipMemcpy(index, c->d_index + (size_t)first * c->data_width, (size_t)n * c->data_width * sizeof(int32_t), hipMemcpyDeviceToHost)); }
    }
    else if (zoomed || index) {
        return fail(c, SDRPP_ERR_INVALID, "no view configured (sdrpp_fft_set_view)");
    }
    return n;
}

int sdrpp_fft_copy_device(sdrpp_ctx* c, int first, int n, float* raw, float* zoomed, int32_t* index) {
    DeviceScope dev_scope_(c);
    if (!c || first < 0 || n < 0) { return SDRPP_ERR_INVALID; }
    FLUSH_PENDING(c);
    if (first >= c->n_lines) { return 0; }
    n = std::min(n, c->n_lines - first);
    if (raw) { HIPCHK(c, hipMemcpyAsync(raw, c->d_lines + (size_t)first * c->fft_size, (size_t)n * c->fft_size * sizeof(float), hipMemcpyDeviceToDevice, c->stream)); }
    if ((zoomed || index) && c->data_width <= 0) { return fail(c, SDRPP_ERR_INVALID, "no view configured (sdrpp_fft_set_view)"); }
    if (zoomed) { HIPCHK(c, hipMemcpyAsync(zoomed, c->d_zoomed + (size_t)first * c->data_width, (size_t)n * c->data_width * sizeof(float), hipMemcpyDeviceToDevice, c->stream)); }
    if (index) { HIPCHK(c, hipMemcpyAsync(index, c->d_index + (size_t)first * c->data_width, (size_t)n * c->data_width * sizeof(int32_t), hipMemcpyDeviceToDevice, c->stream)); }
    return n;
}

int sdrpp_fft_device_buffers(sdrpp_ctx* c, const float** raw, const float** zoomed, const int32_t** index, int* n_lines) {
    DeviceScope dev_scope_(c);
    if (!c) { return SDRPP_ERR_INVALID; }
    FLUSH_PENDING(c);
    if (raw) { *raw = c->d_lines; }
    if (zoomed) { *zoomed = c->d_zoomed; }
    if (index) { *index = c->d_index; }
    if (n_lines) { *n_lines = c->n_lines; }
    return SDRPP_OK;
}

int sdrpp_preproc_configure(sdrpp_ctx* c, int n_stages, const int* stage_decim, const int* stage_ntaps, const float* const* stage_taps, float dc_rate, int conjugate) {
    DeviceScope dev_scope_(c);
    if (!c || n_stages < 0 || n_stages > SDRPP_MAX_DECIM_STAGES) { return SDRPP_ERR_INVALID; }
    FLUSH_PENDING(c);
    const RateDesc rd = rate_desc(n_stages, stage_decim, stage_ntaps, stage_taps);
    if (int rc = rate_check_stages(c, rd, "pre-processing ")) { return rc; }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    preproc_free(c);
    if (n_stages == 0 && dc_rate == 0.0f && !conjugate) { return SDRPP_OK; }  // chain fully disabled: pushes go straight through
    sdrpp_ctx::Pre& P = c->pre;
    RateChain& R = P.rate;
    rate_describe(R, rd);
    P.ref_order = c->pre_ref_order;
    P.dc_rate = dc_rate;
    P.conj = conjugate ? 1 : 0;
    int rc;
    size_t cap = (size_t)c->max_push;
    if (n_stages > 0) {
        P.raw.width = 2;
        P.raw.hist_len = R.need(0, 0);
        for (int i = 0; i < 2; i++) {
            rc = dev_alloc(c, &P.raw.hist[i], (size_t)std::max(P.raw.hist_len, 1) * 2);
            if (rc) { return rc; }
            HIPCHK(c, hipMemset(P.raw.hist[i], 0, (size_t)std::max(P.raw.hist_len, 1) * 2 * sizeof(float)));
        }
    }
    if ((rc = rate_build(c, R, RateForm{}, P.st, cap, 0))) { return rc; }
    if (dc_rate != 0.0f || conjugate) {
        rc = stream_alloc(c, P.out, 2, 0, cap);
        if (rc) { return rc; }
    }
    if (dc_rate != 0.0f) {
        rc = dev_alloc(c, &P.d_off, 2);
        if (rc) { return rc; }
        HIPCHK(c, hipMemset(P.d_off, 0, 2 * sizeof(float2)));
        P.state_cur = 0;
        P.seg_cap = (int)(cap / SDRPP_DEEMP_SEG) + 2;
        rc = dev_alloc(c, &P.d_seg, 2 * ((size_t)P.seg_cap + 1));
        if (rc) { return rc; }
    }
    P.on = true;
    return SDRPP_OK;
}

// IQFrontEnd's setters re-plan the chain but its blocks live on (iq_frontend.cpp:76-130): setSampleRate / setDCBlocking / setInvertIQ do not touch
// the decimator (its delay lines stay), and the DC blocker keeps its estimate through everything — setRate only swaps the rate, a blocker that
// is switched off and on again continues from where it was (dc_blocker.h: the object is only taken out of the chain).  setDecimation creates
// new decimator stages (PowerDecimator::setRatio -> reconfigure: power_decimator.h:91-108): cleared delay lines.
//   keep & 1: the decimator's delay lines and offsets, if the new description has the same stages;   keep & 2: the DC blocker's estimate
int sdrpp_preproc_reconfigure(sdrpp_ctx* c, int n_stages, const int* stage_decim, const int* stage_ntaps, const float* const* stage_taps, float dc_rate, int conjugate, int keep) {
    DeviceScope dev_scope_(c);
    if (!c || n_stages < 0 || n_stages > SDRPP_MAX_DECIM_STAGES || keep < 0 || keep > 3) { return SDRPP_ERR_INVALID; }
    FLUSH_PENDING(c);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    sdrpp_ctx::Pre& P = c->pre;
    if (P.on && P.dc_rate != 0.0f && P.d_off) { HIPCHK(c, hipMemcpy(&c->pre_dc_last, P.d_off + P.state_cur, sizeof(float2), hipMemcpyDeviceToHost)); }
    const bool same = (keep & 1) && P.on && n_stages > 0 && rate_same(P.rate, rate_desc(n_stages, stage_decim, stage_ntaps, stage_taps));
    sdrpp_ctx::Pre old;
    if (same) {  // set the decimator's streams (delay lines, ring buffers) and offsets aside; the rest of the old chain is freed by the configure below
        std::swap(old.raw, P.raw);
        std::swap(old.st, P.st);
        old.rate.pos = P.rate.pos;
    }
    int rc = sdrpp_preproc_configure(c, n_stages, stage_decim, stage_ntaps, stage_taps, dc_rate, conjugate);
    if (same) {
        if (!rc && P.on) {
            std::swap(old.raw, P.raw);
            std::swap(old.st, P.st);
            P.rate.pos = old.rate.pos;
        }
        old.raw.data = nullptr;
        stream_free(old.raw);
        for (auto& st : old.st) { stream_free(st); }
    }
    if (rc) { return rc; }
    if ((keep & 2) && P.on && P.dc_rate != 0.0f && P.d_off) { HIPCHK(c, hipMemcpy(P.d_off + P.state_cur, &c->pre_dc_last, sizeof(float2), hipMemcpyHostToDevice)); }
    if (!(keep & 2)) { c->pre_dc_last = make_float2(0.0f, 0.0f); }
    return SDRPP_OK;
}

int sdrpp_preproc_set_reference_order(sdrpp_ctx* c, int on) {
    DeviceScope dev_scope_(c);
    if (!c) { return SDRPP_ERR_INVALID; }
    FLUSH_PENDING(c);
    c->pre_ref_order = on != 0;
    c->pre.ref_order = c->pre_ref_order;
    return SDRPP_OK;
}

int sdrpp_preproc_out_count(sdrpp_ctx* c) {
    DeviceScope dev_scope_(c);
    if (!c) { return SDRPP_ERR_INVALID; }
    FLUSH_PENDING(c);
    return out_count(c, out_of_preproc(c), kNoPreproc, 0);
}

int sdrpp_preproc_read(sdrpp_ctx* c, float* dst, int max) {
    DeviceScope dev_scope_(c);
    if (!c || !dst || max < 0) { return SDRPP_ERR_INVALID; }
    FLUSH_PENDING(c);
    return out_read(c, out_of_preproc(c), kNoPreproc, 0, dst, max, false);
}

int sdrpp_preproc_device_buffer(sdrpp_ctx* c, const float** iq, int* n) {
    DeviceScope dev_scope_(c);
    if (!c) { return SDRPP_ERR_INVALID; }
    FLUSH_PENDING(c);
    return out_hand(c, out_of_preproc(c), kNoPreproc, 0, iq, n);
}

// ---- VFOs ----------------------------------------------------------------------------------------------------------------------
int sdrpp_vfo_add(sdrpp_ctx* c, const sdrpp_vfo_desc* d, int* id) {
    DeviceScope dev_scope_(c);
    if (!c || !d || !id) { return SDRPP_ERR_INVALID; }
    FLUSH_PENDING(c);
    return vfo_build(c, d, id);
}

int sdrpp_vfo_remove(sdrpp_ctx* c, int id) {
    DeviceScope dev_scope_(c);
    if (!c) { return SDRPP_ERR_INVALID; }
    FLUSH_PENDING(c);
    LOOKUP_VFO(v, c, id);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    rds_detach(c, *v);
    sym_detach(c, *v);
    rdsd_detach(c, *v);
    qpsk_detach(c, *v);
    vfo_free(*v);
    c->vfos.erase(id);
    vfo_list_rebuild(c);
    return SDRPP_OK;
}

int sdrpp_vfo_count(sdrpp_ctx* c) { return c ? (int)c->vfos.size() : SDRPP_ERR_INVALID; }

int sdrpp_vfo_replace(sdrpp_ctx* c, int old_id, const sdrpp_vfo_desc* d, int keep, int* new_id) {
    DeviceScope dev_scope_(c);
    if (!c || !d || !new_id || keep < 0 || keep > 7) { return SDRPP_ERR_INVALID; }
    FLUSH_PENDING(c);
    LOOKUP_VFO(o, c, old_id);
    int nid = 0;
    int rc = vfo_build(c, d, &nid);
    if (rc) { return rc; }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if ((rc = vfo_hand_over(c, *o, *c->vfos[nid], keep))) { return rc; }
    if ((rc = sdrpp_vfo_remove(c, old_id))) { return rc; }
    *new_id = nid;
    return SDRPP_OK;
}

int sdrpp_vfo_set_phase_delta(sdrpp_ctx* c, int id, float re, float im) {
    DeviceScope dev_scope_(c);
    if (!c) { return SDRPP_ERR_INVALID; }
    FLUSH_PENDING(c);
    LOOKUP_VFO(v, c, id);
    const double th = sdrpp_host::turnsPerSample(re, im);
    // the samples already in the first decimator's delay line stay rotated with the old increment (rx_vfo.h:72-77 only swaps
    // phaseDelta): remember where it changed so the first outputs of the next pushes can be handed over exactly (do_vfos)
    if (!v->nco_exact && v->rate.n_stages > 0 && th != v->theta) {
        if (!v->recs.empty() && v->recs.back().pos == v->seen) { /* retuned twice between pushes: the older increment stays the one before */ }
        else { v->recs.push_back(Vfo::Retune{ v->seen, v->theta }); }
    }
    v->d.phase_delta_re = re;
    v->d.phase_delta_im = im;
    v->theta = th;
    v->modtaps_dirty = true;
    return SDRPP_OK;
}

int sdrpp_vfo_set_channel_taps(sdrpp_ctx* c, int id, const float* taps, int n) {
    DeviceScope dev_scope_(c);
    if (!c || n < 0 || (n > 0 && !taps)) { return SDRPP_ERR_INVALID; }
    if (n > kChanMaxTaps) { return fail(c, SDRPP_ERR_UNSUPPORTED, "channel filter of %d taps (max %d)", n, kChanMaxTaps); }
    FLUSH_PENDING(c);
    LOOKUP_VFO(v, c, id);
    return vfo_set_chan_taps(c, *v, taps, n);
}

int sdrpp_vfo_set_af(sdrpp_ctx* c, int id, const sdrpp_af_desc* af) {
    DeviceScope dev_scope_(c);
    if (!c) { return SDRPP_ERR_INVALID; }
    FLUSH_PENDING(c);
    LOOKUP_VFO(v, c, id);
    return af_apply(c, *v, af);
}

int sdrpp_vfo_af_count(sdrpp_ctx* c, int id) {
    DeviceScope dev_scope_(c);
    if (!c) { return SDRPP_ERR_INVALID; }
    FLUSH_PENDING(c);
    LOOKUP_VFO(v, c, id);
    return out_count(c, out_of(delivered(*v, 2)), kNoAf, id);
}

int sdrpp_vfo_af_read(sdrpp_ctx* c, int id, float* dst, int max) {
    DeviceScope dev_scope_(c);
    if (!c || !dst || max < 0) { return SDRPP_ERR_INVALID; }
    FLUSH_PENDING(c);
    LOOKUP_VFO(v, c, id);
    return out_read(c, out_of(delivered(*v, 2)), kNoAf, id, dst, max, true);
}

int sdrpp_vfo_af_device_buffer(sdrpp_ctx* c, int id, const float** out, int* n_out) {
    DeviceScope dev_scope_(c);
    if (!c) { return SDRPP_ERR_INVALID; }
    FLUSH_PENDING(c);
    LOOKUP_VFO(v, c, id);
    return out_hand(c, out_of(delivered(*v, 2)), kNoAf, id, out, n_out);
}

int sdrpp_abi_sizeof_af_desc(void) { return (int)sizeof(sdrpp_af_desc); }

// ---- radio IF chain: NoiseBlanker -> PowerSquelch between RxVFO::out and the demodulator (radio_module.h:84-96) ---------------------
int sdrpp_vfo_set_if(sdrpp_ctx* c, int id, const sdrpp_if_desc* d) {
    DeviceScope dev_scope_(c);
    if (!c) { return SDRPP_ERR_INVALID; }
    FLUSH_PENDING(c);
    LOOKUP_VFO(v, c, id);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return ifc_apply(c, *v, d);
}

// ... and its last block, FMIF (the FM IF noise reduction), switched by a call of its own
int sdrpp_vfo_set_fmnr(sdrpp_ctx* c, int id, int enabled, int bins) {
    DeviceScope dev_scope_(c);
    if (!c) { return SDRPP_ERR_INVALID; }
    FLUSH_PENDING(c);
    if (bins > kFmifTile) { return fail(c, SDRPP_ERR_UNSUPPORTED, "FMIF with %d bins (the matrix tile holds %d)", bins, kFmifTile); }
    if (bins < 2) { return fail(c, SDRPP_ERR_INVALID, "FMIF with %d bins", bins); }
    LOOKUP_VFO(v, c, id);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return fmnr_apply(c, *v, enabled != 0, bins);
}

int sdrpp_vfo_ifc_count(sdrpp_ctx* c, int id) {
    DeviceScope dev_scope_(c);
    if (!c) { return SDRPP_ERR_INVALID; }
    FLUSH_PENDING(c);
    LOOKUP_VFO(v, c, id);
    return out_count(c, out_of(delivered(*v, 3)), kNoIfc, id);
}

int sdrpp_vfo_ifc_read(sdrpp_ctx* c, int id, float* dst, int max) {
    DeviceScope dev_scope_(c);
    if (!c || !dst || max < 0) { return SDRPP_ERR_INVALID; }
    FLUSH_PENDING(c);
    LOOKUP_VFO(v, c, id);
    return out_read(c, out_of(delivered(*v, 3)), kNoIfc, id, dst, max, true);
}

int sdrpp_vfo_ifc_device_buffer(sdrpp_ctx* c, int id, const float** out, int* n_out) {
    DeviceScope dev_scope_(c);
    if (!c) { return SDRPP_ERR_INVALID; }
    FLUSH_PENDING(c);
    LOOKUP_VFO(v, c, id);
    return out_hand(c, out_of(delivered(*v, 3)), kNoIfc, id, out, n_out);
}

int sdrpp_abi_sizeof_if_desc(void) { return (int)sizeof(sdrpp_if_desc); }

// ---- recorder sink: volume -> peak meter -> optional mono fold -> the file's sample type (misc_modules/recorder) --------------------------
int sdrpp_vfo_set_rec(sdrpp_ctx* c, int id, const sdrpp_rec_desc* d) {
    DeviceScope dev_scope_(c);
    if (!c) { return SDRPP_ERR_INVALID; }
    FLUSH_PENDING(c);
    LOOKUP_VFO(v, c, id);
    return rec_apply(c, *v, d);
}

int sdrpp_vfo_rec_read(sdrpp_ctx* c, int id, void* dst_host, int max_frames, sdrpp_rec_info* info) {
    DeviceScope dev_scope_(c);
    if (!c || max_frames < 0 || (max_frames > 0 && !dst_host)) { return SDRPP_ERR_INVALID; }
    FLUSH_PENDING(c);
    LOOKUP_VFO(v, c, id);
    return rec_read(c, *v, dst_host, max_frames, info);
}

int sdrpp_abi_sizeof_rec_desc(void) { return (int)sizeof(sdrpp_rec_desc); }

// ---- RDS branch of the WFM demodulator: discriminator -> translation by -57 kHz -> resampler to 5 kS/s (broadcast_fm.h:144-215) -----------------
int sdrpp_vfo_set_rds(sdrpp_ctx* c, int id, const sdrpp_rds_desc* d, int enabled) {
    DeviceScope dev_scope_(c);
    if (!c) { return SDRPP_ERR_INVALID; }
    FLUSH_PENDING(c);
    LOOKUP_VFO(v, c, id);
    if (!d) { return rds_apply(c, *v, nullptr, 0.0f, 0.0f, false); }
    const RateDesc rd = rate_desc(*d);
    return rds_apply(c, *v, &rd, d->phase_delta_re, d->phase_delta_im, enabled != 0);
}

// ---- stereo branch of the WFM demodulator: pilot filter -> PLL -> L-R matrix -> L / R low-pass (broadcast_fm.h:147-191) ---------------------------
int sdrpp_vfo_set_stereo(sdrpp_ctx* c, int id, const sdrpp_stereo_desc* d) {
    DeviceScope dev_scope_(c);
    if (!c) { return SDRPP_ERR_INVALID; }
    FLUSH_PENDING(c);
    LOOKUP_VFO(v, c, id);
    return stereo_apply(c, *v, d);
}
int sdrpp_abi_sizeof_stereo_desc(void) { return (int)sizeof(sdrpp_stereo_desc); }

int sdrpp_vfo_rds_count(sdrpp_ctx* c, int id) {
    DeviceScope dev_scope_(c);
    if (!c) { return SDRPP_ERR_INVALID; }
    FLUSH_PENDING(c);
    LOOKUP_VFO(v, c, id);
    return out_count(c, out_of_rds(*v), kNoRds, id);
}

int sdrpp_vfo_rds_read(sdrpp_ctx* c, int id, float* dst, int max) {
    DeviceScope dev_scope_(c);
    if (!c || !dst || max < 0) { return SDRPP_ERR_INVALID; }
    FLUSH_PENDING(c);
    LOOKUP_VFO(v, c, id);
    return out_read(c, out_of_rds(*v), kNoRds, id, dst, max, false);
}

int sdrpp_vfo_rds_device_buffer(sdrpp_ctx* c, int id, const float** out, int* n_out) {
    DeviceScope dev_scope_(c);
    if (!c) { return SDRPP_ERR_INVALID; }
    FLUSH_PENDING(c);
    LOOKUP_VFO(v, c, id);
    return out_hand(c, out_of_rds(*v), kNoRds, id, out, n_out);
}

int sdrpp_abi_sizeof_rds_desc(void) { return (int)sizeof(sdrpp_rds_desc); }
int sdrpp_rds_bank_count(sdrpp_ctx* c) { return c ? (int)c->rds_banks.size() : SDRPP_ERR_INVALID; }

// ---- symbol branch of a RAW VFO: discriminator -> shaping FIR -> MM clock recovery -> soft symbols, bits (pocsag/dsp.h, clock_recovery/mm.h) -----------
int sdrpp_vfo_set_symbols(sdrpp_ctx* c, int id, const sdrpp_sym_desc* d, int enabled) {
    DeviceScope dev_scope_(c);
    if (!c) { return SDRPP_ERR_INVALID; }
    FLUSH_PENDING(c);
    LOOKUP_VFO(v, c, id);
    return sym_apply(c, *v, d, enabled != 0);
}
int sdrpp_vfo_sym_count(sdrpp_ctx* c, int id) {
    DeviceScope dev_scope_(c);
    if (!c) { return SDRPP_ERR_INVALID; }
    FLUSH_PENDING(c);
    LOOKUP_VFO(v, c, id);
    return sym_count(c, *v);
}
int sdrpp_vfo_sym_read(sdrpp_ctx* c, int id, float* soft, uint8_t* bits, int max) {
    DeviceScope dev_scope_(c);
    if (!c || max < 0) { return SDRPP_ERR_INVALID; }
    FLUSH_PENDING(c);
    LOOKUP_VFO(v, c, id);
    const int have = sym_count(c, *v);
    if (have < 0) { return have; }
    const int n = std::min(have, max);
    if (n > 0 && soft) { HIPCHK(c, hipMemcpy(soft, v->sym.st[1].data, (size_t)n * sizeof(float), hipMemcpyDeviceToHost)); }
    if (n > 0 && bits) { HIPCHK(c, hipMemcpy(bits, v->sym.st[2].data, (size_t)n, hipMemcpyDeviceToHost)); }
    return n;
}
int sdrpp_vfo_sym_device_buffers(sdrpp_ctx* c, int id, const float** soft, const uint8_t** bits, int* n) {
    DeviceScope dev_scope_(c);
    if (!c) { return SDRPP_ERR_INVALID; }
    FLUSH_PENDING(c);
    LOOKUP_VFO(v, c, id);
    const int have = sym_count(c, *v);
    if (have < 0) { return have; }
    if (soft) { *soft = v->sym.st[1].data; }
    if (bits) { *bits = reinterpret_cast<const uint8_t*>(v->sym.st[2].data); }
    if (n) { *n = have; }
    return SDRPP_OK;
}
int sdrpp_abi_sizeof_sym_desc(void) { return (int)sizeof(sdrpp_sym_desc); }
int sdrpp_sym_bank_count(sdrpp_ctx* c) { return c ? (int)c->sym_banks.size() : SDRPP_ERR_INVALID; }

// ---- framer behind the symbol branch: 4FSK slicer -> sync search -> descrambled, de-interleaved frames (m17_decoder/src/m17dsp.h) -----------------------
int sdrpp_vfo_set_framer(sdrpp_ctx* c, int id, const sdrpp_frame_desc* d, int enabled) {
    DeviceScope dev_scope_(c);
    if (!c) { return SDRPP_ERR_INVALID; }
    FLUSH_PENDING(c);
    LOOKUP_VFO(v, c, id);
    return frame_apply(c, *v, d, enabled != 0);
}
int sdrpp_vfo_framer_reset(sdrpp_ctx* c, int id) {
    DeviceScope dev_scope_(c);
    if (!c) { return SDRPP_ERR_INVALID; }
    FLUSH_PENDING(c);
    LOOKUP_VFO(v, c, id);
    return frame_reset(c, *v);
}
int sdrpp_vfo_frame_count(sdrpp_ctx* c, int id) {
    DeviceScope dev_scope_(c);
    if (!c) { return SDRPP_ERR_INVALID; }
    FLUSH_PENDING(c);
    LOOKUP_VFO(v, c, id);
    return frame_count(c, *v);
}
int sdrpp_vfo_frame_read(sdrpp_ctx* c, int id, uint8_t* records, int max_frames) {
    DeviceScope dev_scope_(c);
    if (!c || max_frames < 0) { return SDRPP_ERR_INVALID; }
    FLUSH_PENDING(c);
    LOOKUP_VFO(v, c, id);
    const int have = frame_count(c, *v);
    if (have < 0) { return have; }
    const int n = std::min(have, max_frames);
    if (n > 0 && records) { HIPCHK(c, hipMemcpy(records, v->frame.st[0].data, (size_t)n * (size_t)v->frame.stride, hipMemcpyDeviceToHost)); }
    return n;
}
int sdrpp_vfo_frame_device_buffer(sdrpp_ctx* c, int id, const uint8_t** records, int* n) {
    DeviceScope dev_scope_(c);
    if (!c) { return SDRPP_ERR_INVALID; }
    FLUSH_PENDING(c);
    LOOKUP_VFO(v, c, id);
    const int have = frame_count(c, *v);
    if (have < 0) { return have; }
    if (records) { *records = reinterpret_cast<const uint8_t*>(v->frame.st[0].data); }
    if (n) { *n = have; }
    return SDRPP_OK;
}
int sdrpp_abi_sizeof_frame_desc(void) { return (int)sizeof(sdrpp_frame_desc); }
int sdrpp_frame_record_stride(int frame_bits) {
    if (frame_bits < 8 || frame_bits > SDRPP_FRAME_MAX_BITS || frame_bits % 8 != 0) { return SDRPP_ERR_INVALID; }
    return frame_record_stride(frame_bits);
}
int sdrpp_frame_table_count(sdrpp_ctx* c) { return c ? (int)c->frame_tabs.size() : SDRPP_ERR_INVALID; }

// ---- RDS demodulator: AGC -> Costas -> band-pass -> Costas -> MM clock recovery -> slicer -> differential decoder (radio/src/rds_demod.h) -----------------
int sdrpp_vfo_set_rds_demod(sdrpp_ctx* c, int id, const sdrpp_rdsd_desc* d, int enabled) {
    DeviceScope dev_scope_(c);
    if (!c) { return SDRPP_ERR_INVALID; }
    FLUSH_PENDING(c);
    LOOKUP_VFO(v, c, id);
    return rdsd_apply(c, *v, d, enabled != 0);
}
int sdrpp_vfo_rds_demod_reset(sdrpp_ctx* c, int id) {
    DeviceScope dev_scope_(c);
    if (!c) { return SDRPP_ERR_INVALID; }
    FLUSH_PENDING(c);
    LOOKUP_VFO(v, c, id);
    if (!v->rdsd.attached) { return fail(c, SDRPP_ERR_INVALID, kNoRdsd, id); }
    return rdsd_clear(c, *v, false);
}
int sdrpp_vfo_rds_demod_count(sdrpp_ctx* c, int id) {
    DeviceScope dev_scope_(c);
    if (!c) { return SDRPP_ERR_INVALID; }
    FLUSH_PENDING(c);
    LOOKUP_VFO(v, c, id);
    return rdsd_count(c, *v);
}
int sdrpp_vfo_rds_demod_read(sdrpp_ctx* c, int id, float* soft, uint8_t* bits, int max) {
    DeviceScope dev_scope_(c);
    if (!c || max < 0) { return SDRPP_ERR_INVALID; }
    FLUSH_PENDING(c);
    LOOKUP_VFO(v, c, id);
    const int have = rdsd_count(c, *v);
    if (have < 0) { return have; }
    const int n = std::min(have, max);
    if (n > 0 && soft) { HIPCHK(c, hipMemcpy(soft, v->rdsd.st[0].data, (size_t)n * sizeof(float), hipMemcpyDeviceToHost)); }
    if (n > 0 && bits) { HIPCHK(c, hipMemcpy(bits, v->rdsd.st[1].data, (size_t)n, hipMemcpyDeviceToHost)); }
    return n;
}
int sdrpp_vfo_rds_demod_device_buffers(sdrpp_ctx* c, int id, const float** soft, const uint8_t** bits, int* n) {
    DeviceScope dev_scope_(c);
    if (!c) { return SDRPP_ERR_INVALID; }
    FLUSH_PENDING(c);
    LOOKUP_VFO(v, c, id);
    const int have = rdsd_count(c, *v);
    if (have < 0) { return have; }
    if (soft) { *soft = v->rdsd.st[0].data; }
    if (bits) { *bits = reinterpret_cast<const uint8_t*>(v->rdsd.st[1].data); }
    if (n) { *n = have; }
    return SDRPP_OK;
}
int sdrpp_abi_sizeof_rdsd_desc(void) { return (int)sizeof(sdrpp_rdsd_desc); }
int sdrpp_rdsd_bank_count(sdrpp_ctx* c) { return c ? (int)c->rdsd_banks.size() : SDRPP_ERR_INVALID; }

// ---- Meteor QPSK demodulator: RRC FIR -> AGC -> QPSK Costas loop -> OQPSK delay -> complex MM (meteor_demodulator/src/meteor_demod.h) --------------------
int sdrpp_vfo_set_qpsk(sdrpp_ctx* c, int id, const sdrpp_qpsk_desc* d, int enabled) {
    DeviceScope dev_scope_(c);
    if (!c) { return SDRPP_ERR_INVALID; }
    FLUSH_PENDING(c);
    LOOKUP_VFO(v, c, id);
    return qpsk_apply(c, *v, d, enabled != 0);
}
int sdrpp_vfo_qpsk_set_mode(sdrpp_ctx* c, int id, int broken, int oqpsk) {
    DeviceScope dev_scope_(c);
    if (!c) { return SDRPP_ERR_INVALID; }
    FLUSH_PENDING(c);
    LOOKUP_VFO(v, c, id);
    if (!v->qpsk.attached) { return fail(c, SDRPP_ERR_INVALID, kNoQpsk, id); }
    v->qpsk.broken = broken != 0;
    v->qpsk.oqpsk = oqpsk != 0;
    return SDRPP_OK;
}
int sdrpp_vfo_qpsk_reset(sdrpp_ctx* c, int id) {
    DeviceScope dev_scope_(c);
    if (!c) { return SDRPP_ERR_INVALID; }
    FLUSH_PENDING(c);
    LOOKUP_VFO(v, c, id);
    if (!v->qpsk.attached) { return fail(c, SDRPP_ERR_INVALID, kNoQpsk, id); }
    return qpsk_clear(c, *v, false);
}
int sdrpp_vfo_qpsk_count(sdrpp_ctx* c, int id) {
    DeviceScope dev_scope_(c);
    if (!c) { return SDRPP_ERR_INVALID; }
    FLUSH_PENDING(c);
    LOOKUP_VFO(v, c, id);
    return qpsk_count(c, *v);
}
int sdrpp_vfo_qpsk_read(sdrpp_ctx* c, int id, float* soft_iq, int8_t* packed, int max) {
    DeviceScope dev_scope_(c);
    if (!c || max < 0) { return SDRPP_ERR_INVALID; }
    FLUSH_PENDING(c);
    LOOKUP_VFO(v, c, id);
    const int have = qpsk_count(c, *v);
    if (have < 0) { return have; }
    const int n = std::min(have, max);
    if (n > 0 && soft_iq) { HIPCHK(c, hipMemcpy(soft_iq, v->qpsk.st[1].data, (size_t)n * 2 * sizeof(float), hipMemcpyDeviceToHost)); }
    if (n > 0 && packed) { HIPCHK(c, hipMemcpy(packed, v->qpsk.st[2].data, (size_t)n * 2, hipMemcpyDeviceToHost)); }
    return n;
}
int sdrpp_vfo_qpsk_device_buffers(sdrpp_ctx* c, int id, const float** soft_iq, const int8_t** packed, int* n) {
    DeviceScope dev_scope_(c);
    if (!c) { return SDRPP_ERR_INVALID; }
    FLUSH_PENDING(c);
    LOOKUP_VFO(v, c, id);
    const int have = qpsk_count(c, *v);
    if (have < 0) { return have; }
    if (soft_iq) { *soft_iq = v->qpsk.st[1].data; }
    if (packed) { *packed = reinterpret_cast<const int8_t*>(v->qpsk.st[2].data); }
    if (n) { *n = have; }
    return SDRPP_OK;
}
int sdrpp_abi_sizeof_qpsk_desc(void) { return (int)sizeof(sdrpp_qpsk_desc); }
int sdrpp_qpsk_bank_count(sdrpp_ctx* c) { return c ? (int)c->qpsk_banks.size() : SDRPP_ERR_INVALID; }

int sdrpp_vfo_read_pcm(sdrpp_ctx* c, int id, int which, int pcm_type, float scale, void* dst_host, int max_frames) {
    DeviceScope dev_scope_(c);
    if (!c || !dst_host || max_frames < 0 || (pcm_type != 0 && pcm_type != 1)) { return SDRPP_ERR_INVALID; }
    FLUSH_PENDING(c);
    LOOKUP_VFO(v, c, id);
    Stream* s = delivered(*v, which);
    if (!s) { return fail(c, SDRPP_ERR_INVALID, "VFO %d has no such stream (%d)", id, which); }
    return pcm_read(c, s->data, s->n, pcm_type, scale, dst_host, max_frames);
}

// the pre-processed wideband IQ of the most recent push as int16 / int8: what the recorder's baseband mode writes (bindIQStream consumer ->
// wav::Writer::write, utils/wav.cpp:158-167)
int sdrpp_preproc_read_pcm(sdrpp_ctx* c, int pcm_type, float scale, void* dst_host, int max_samples) {
    DeviceScope dev_scope_(c);
    if (!c || !dst_host || max_samples < 0 || (pcm_type != 0 && pcm_type != 1)) { return SDRPP_ERR_INVALID; }
    FLUSH_PENDING(c);
    if (!c->pre.on) { return fail(c, SDRPP_ERR_INVALID, kNoPreproc); }
    return pcm_read(c, c->pre.last, c->pre.last_n, pcm_type, scale, dst_host, max_samples);
}

int sdrpp_vfo_read_compressed(sdrpp_ctx* c, int id, int which, int pcm_type, unsigned char* dst_host, int max_bytes) {
    DeviceScope dev_scope_(c);
    if (!c || !dst_host || pcm_type < 0 || pcm_type > 2) { return SDRPP_ERR_INVALID; }
    FLUSH_PENDING(c);
    LOOKUP_VFO(v, c, id);
    Stream* s = delivered(*v, which);
    if (!s) { return fail(c, SDRPP_ERR_INVALID, "VFO %d has no such stream (%d)", id, which); }
    const int n = s->n;
    const long long nv = (long long)n * 2;
    const size_t esz = pcm_type == 2 ? 4 : (pcm_type == 1 ? 2 : 1);
    const size_t total = 8 + (size_t)nv * esz;
    if (n == 0) { return 0; }  // the reference block does not swap an empty frame (sample_stream_compressor.h:70-73)
    if ((size_t)max_bytes < total) { return fail(c, SDRPP_ERR_INVALID, "compressed frame needs %zu bytes", total); }
    uint16_t hdr[2] = { 0, (uint16_t)pcm_type };
    memcpy(dst_host, hdr, 4);
    float scaler = 0.0f;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (pcm_type == 2) {
        memcpy(dst_host + 4, &scaler, 4);
        HIPCHK(c, hipMemcpy(dst_host + 8, s->data, (size_t)nv * 4, hipMemcpyDeviceToHost));
        return (int)total;
    }
    int rc = pack_scratch(c, (size_t)nv * esz + 256 * sizeof(float));
    if (rc) { return rc; }
    float* d_part = (float*)(c->d_pack);
    char* d_data = c->d_pack + 256 * sizeof(float);
    const int nb = (int)std::min<long long>((nv + 255) / 256, 256);
    hipLaunchKernelGGL(pack_max_kernel, dim3((unsigned)nb), dim3(256), 0, c->stream, (const float*)s->data, nv, d_part);
    float part[256];
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(part, d_part, (size_t)nb * sizeof(float), hipMemcpyDeviceToHost));
    float maxVal = part[0];
    for (int i = 1; i < nb; i++) {
        if (part[i] > maxVal) { maxVal = part[i]; }
    }
    scaler = maxVal;
    memcpy(dst_host + 4, &scaler, 4);
    pack_convert(c, s->data, nv, (pcm_type == 1 ? 32768.0f : 128.0f) / maxVal, pcm_type, d_data);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(dst_host + 8, d_data, (size_t)nv * esz, hipMemcpyDeviceToHost));
    return (int)total;
}

// calculateVFOSignalInfo (waterfall.cpp:558-598) on the newest line of the history ring
int sdrpp_wf_signal_info(sdrpp_ctx* c, double center_offset, double bandwidth, double whole_bandwidth, float* strength, float* snr) {
    DeviceScope dev_scope_(c);
    if (!c || !strength || !snr) { return SDRPP_ERR_INVALID; }
    FLUSH_PENDING(c);
    sdrpp_ctx::Wf& W = c->wf;
    if (W.height <= 0) { return fail(c, SDRPP_ERR_INVALID, "no waterfall history configured (sdrpp_wf_configure)"); }
    if (W.lines <= 0) { return 0; }  // the reference returns false: nothing to measure yet
    const int N = c->fft_size;
    const WfMeterOffs o = wf_meter_offsets(center_offset, bandwidth, whole_bandwidth, N);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (c->fft_stream) { HIPCHK(c, hipStreamSynchronize(c->fft_stream)); }
    int rc = pack_scratch(c, 64);
    if (rc) { return rc; }
    hipLaunchKernelGGL(wf_signal_info_kernel, dim3(1), dim3(256), 0, c->stream, (const float*)(W.d_ring + (size_t)W.cur * N), o.o0, o.o1, o.o2, o.o3, (float*)c->d_pack);
    float out[2];
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(out, c->d_pack, sizeof(out), hipMemcpyDeviceToHost));
    *strength = out[0];
    *snr = out[1];
    return 1;
}

// ---- signal meters: a table of bands on every line of every push (plan_fft.h: wf_meter_offsets / run_meters; tick_host.h: the result slots) ----
int sdrpp_wf_set_meters(sdrpp_ctx* c, int n, const sdrpp_meter_desc* descs, double whole_bandwidth) {
    DeviceScope dev_scope_(c);
    if (!c || n < 0 || (n > 0 && !descs)) { return SDRPP_ERR_INVALID; }
    if (!c->fft_on) { return fail(c, SDRPP_ERR_INVALID, "sdrpp_wf_set_meters: no FFT configured (sdrpp_fft_configure)"); }
    if (n > SDRPP_MAX_METERS) { return fail(c, SDRPP_ERR_UNSUPPORTED, "sdrpp_wf_set_meters: %d meters, at most %d", n, SDRPP_MAX_METERS); }
    if (n > 0 && !(whole_bandwidth > 0.0 && std::isfinite(whole_bandwidth))) { return fail(c, SDRPP_ERR_INVALID, "sdrpp_wf_set_meters: whole_bandwidth %g", whole_bandwidth); }
    for (int i = 0; i < n; i++) {
        if (!std::isfinite(descs[i].center_offset) || !std::isfinite(descs[i].bandwidth)) { return fail(c, SDRPP_ERR_INVALID, "sdrpp_wf_set_meters: meter %d is not a finite band", i); }
    }
    // what has been pushed keeps the table it was pushed with: deferred pushes are processed, a held launch group goes out — the tick queue of a
    // pipelined run is left alone (its blocks carry their own copy of the table)
    int rc = flush_pending_opt(c, 0);
    if (rc) { return rc; }
    if (!c->pipelined) {  // an ordinary pass in flight reads the device copy
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (c->fft_stream) { HIPCHK(c, hipStreamSynchronize(c->fft_stream)); }
    }
    c->meters.descs.assign(descs, descs + n);
    c->meters.whole_bandwidth = n > 0 ? whole_bandwidth : 0.0;
    return meters_rebuild(c);
}
int sdrpp_wf_meters_read(sdrpp_ctx* c, float* dst, int max_lines, int* n_lines, int* n_meters) {
    DeviceScope dev_scope_(c);
    if (!c || max_lines < 0) { return SDRPP_ERR_INVALID; }
    if (c->pipelined) { return fail(c, SDRPP_ERR_INVALID, "sdrpp_wf_meters_read: in pipelined mode the meters come with the results (sdrpp_result_meters)"); }
    FLUSH_PENDING(c);
    const sdrpp_ctx::Meters& M = c->meters;
    const int lines = (M.out_n > 0 && M.out_lines == c->n_lines) ? M.out_lines : 0;
    if (n_lines) { *n_lines = lines; }
    if (n_meters) { *n_meters = M.n(); }
    if (!dst || lines == 0) { return SDRPP_OK; }
    if (lines > max_lines) { return fail(c, SDRPP_ERR_INVALID, "sdrpp_wf_meters_read: the push completed %d lines, room for %d", lines, max_lines); }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (c->fft_stream) { HIPCHK(c, hipStreamSynchronize(c->fft_stream)); }
    HIPCHK(c, hipMemcpy(dst, M.d_out, (size_t)lines * M.out_n * 2 * sizeof(float), hipMemcpyDeviceToHost));
    return SDRPP_OK;
}
int sdrpp_abi_sizeof_meter_desc(void) { return (int)sizeof(sdrpp_meter_desc); }

int sdrpp_set_reference_block(sdrpp_ctx* c, int ref_block) {
    DeviceScope dev_scope_(c);
    if (!c || ref_block < 0) { return SDRPP_ERR_INVALID; }
    FLUSH_PENDING(c);
    c->ref_block = ref_block;
    return SDRPP_OK;
}

int sdrpp_set_backend_pipeline(sdrpp_ctx* c, int on) {
    DeviceScope dev_scope_(c);
    if (!c) { return SDRPP_ERR_INVALID; }
    c->pipe_on = on < 0 ? 0 : on;
    return SDRPP_OK;
}
int sdrpp_set_nco_mode(sdrpp_ctx* c, int mode) {
    DeviceScope dev_scope_(c);
    if (!c || (mode != SDRPP_NCO_CLOSED_FORM && mode != SDRPP_NCO_REFERENCE_ROTATOR)) { return SDRPP_ERR_INVALID; }
    FLUSH_PENDING(c);
    if (!c->vfos.empty() && mode != c->nco_exact) { return fail(c, SDRPP_ERR_INVALID, "the NCO mode can only change while no VFO exists (it decides how a VFO's front end is built)"); }
    c->nco_exact = mode;
    return SDRPP_OK;
}

int sdrpp_vfo_set_ssb_phase_delta(sdrpp_ctx* c, int id, float re, float im) {
    DeviceScope dev_scope_(c);
    if (!c) { return SDRPP_ERR_INVALID; }
    FLUSH_PENDING(c);
    LOOKUP_VFO(v, c, id);
    if (v->d.demod < SDRPP_DEMOD_USB) { return fail(c, SDRPP_ERR_INVALID, "VFO %d has no SSB demodulator", id); }  // (USB, LSB, DSB; CW: the tone)
    v->d.ssb_phase_delta_re = re;
    v->d.ssb_phase_delta_im = im;
    v->theta2 = sdrpp_host::turnsPerSample(re, im);  // the translation is sample-wise: nothing to hand over, the phase stays continuous
    return SDRPP_OK;
}

int sdrpp_vfo_reset(sdrpp_ctx* c, int id) {
    DeviceScope dev_scope_(c);
    if (!c) { return SDRPP_ERR_INVALID; }
    FLUSH_PENDING(c);
    LOOKUP_VFO(v, c, id);
    if (int rc = rds_freeze(c, *v)) { return rc; }  // (the RDS branch's delay line is not the demodulator's: it outlives the history cleared below)
    if (int rc = sym_reset_prev(c, *v)) { return rc; }
    return vfo_reset_state(c, *v);
}

int sdrpp_vfo_out_count(sdrpp_ctx* c, int id) {
    DeviceScope dev_scope_(c);
    if (!c) { return SDRPP_ERR_INVALID; }
    if (int frc = flush_pending_opt(c, 0)) { return frc; }  // (non-draining: a count is what the HOST knows)
    LOOKUP_VFO(v, c, id);
    return delivered(*v, 0)->n;
}

int sdrpp_vfo_read(sdrpp_ctx* c, int id, float* dst, int max) {
    DeviceScope dev_scope_(c);
    if (!c || !dst || max < 0) { return SDRPP_ERR_INVALID; }
    FLUSH_PENDING(c);
    LOOKUP_VFO(v, c, id);
    return out_read(c, out_of(delivered(*v, 0)), kNoOut, id, dst, max, true);
}

int sdrpp_vfo_read_many(sdrpp_ctx* c, int n, const int* ids, const int* which, float* dst_host, int64_t max_samples, int64_t* offsets, int* counts) {
    DeviceScope dev_scope_(c);
    if (!c || n < 0 || (n > 0 && (!ids || !offsets || !counts)) || max_samples < 0) { return SDRPP_ERR_INVALID; }
    FLUSH_PENDING(c);
    std::vector<GatherJob> jobs;
    int64_t total = 0;
    int mx = 0;
    for (int i = 0; i < n; i++) {
        LOOKUP_VFO(v, c, ids[i]);
        Stream* s = delivered(*v, which ? which[i] : 0);
        if (!s) { return fail(c, SDRPP_ERR_INVALID, "VFO %d has no such stream (%d)", ids[i], which ? which[i] : 0); }
        offsets[i] = total;
        counts[i] = s->n;
        if (s->n > 0) { jobs.push_back(GatherJob{ (const float2*)s->data, (long long)total, s->n }); }
        mx = std::max(mx, s->n);
        total += s->n;
    }
    if (!dst_host) { return (int)std::min<int64_t>(total, 0x7fffffff); }  // size query: offsets / counts filled, nothing copied
    if (total > max_samples) { return fail(c, SDRPP_ERR_INVALID, "the outputs need room for %lld samples", (long long)total); }
    if (total == 0) { return 0; }
    if ((size_t)total > c->gather_cap) {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        dev_free(c->d_gather);
        c->gather_cap = 0;
        int rc = dev_alloc(c, &c->d_gather, (size_t)total + 4096);
        if (rc) { return rc; }
        c->gather_cap = (size_t)total + 4096;
    }
    if (jobs.size() <= SDRPP_GATHER_INLINE) {
        GatherArgs ga{};
        for (size_t k = 0; k < jobs.size(); k++) { ga.j[k] = jobs[k]; }
        hipLaunchKernelGGL(gather_inline_kernel, dim3((unsigned)std::max(1, std::min((mx + 255) / 256, 64)), (unsigned)jobs.size()), dim3(256), 0, c->stream, ga, c->d_gather);
        HIPCHK(c, hipMemcpyAsync(dst_host, c->d_gather, (size_t)total * sizeof(float2), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (int rc = pipe_timeouts_check(c)) { return rc; }
        return (int)std::min<int64_t>(total, 0x7fffffff);
    }
    if ((int)jobs.size() > c->gather_jobs_cap) {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        dev_free(c->d_gather_jobs);
        c->gather_jobs_cap = 0;
        int rc = dev_alloc(c, &c->d_gather_jobs, jobs.size() + 64);
        if (rc) { return rc; }
        c->gather_jobs_cap = (int)jobs.size() + 64;
    }
    HIPCHK(c, hipMemcpyAsync(c->d_gather_jobs, jobs.data(), jobs.size() * sizeof(GatherJob), hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(gather_kernel, dim3((unsigned)std::max(1, std::min((mx + 255) / 256, 64)), (unsigned)jobs.size()), dim3(256), 0, c->stream, (const GatherJob*)c->d_gather_jobs, c->d_gather);
    HIPCHK(c, hipMemcpyAsync(dst_host, c->d_gather, (size_t)total * sizeof(float2), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));  // also keeps `jobs` alive until the upload has been consumed
    if (int rc = pipe_timeouts_check(c)) { return rc; }
    return (int)std::min<int64_t>(total, 0x7fffffff);
}

int sdrpp_vfo_device_buffers(sdrpp_ctx* c, int id, const float** out, int* n_out, const float** if_out, int* n_if) {
    DeviceScope dev_scope_(c);
    if (!c) { return SDRPP_ERR_INVALID; }
    FLUSH_PENDING(c);
    LOOKUP_VFO(v, c, id);
    (void)out_hand(c, out_of(delivered(*v, 0)), kNoOut, id, out, n_out);
    return out_hand(c, out_of(delivered(*v, 1)), kNoOut, id, if_out, n_if);
}

// ---- data path --------------------------------------------------------------------------------------------------------------------
// Landing buffer of the pass being assembled (allocated on first use of the second one; waits until the pass that last read it is done)
static int landing_acquire(sdrpp_ctx* c, bool need16) {
    const int b = c->land_cur;
    if (!c->iq_land[b]) {
        int rc = dev_alloc(c, &c->iq_land[b], (size_t)c->max_push * 2 + 32);
        if (rc) { return rc; }
    }
    if (need16 && !c->iq_land16[b]) {
        int rc = dev_alloc(c, &c->iq_land16[b], (size_t)c->max_push * 2 + 32);
        if (rc) { return rc; }
    }
    if (c->pending == 0 && c->land_used[b]) {
        HIPCHK(c, hipEventSynchronize(c->land_ev[b]));
        c->land_used[b] = false;
    }
    return SDRPP_OK;
}
// the pass over what has been staged: kernels enqueued, landing buffer marked busy until they are done, the other one becomes current
static int landing_process(sdrpp_ctx* c, int64_t count, const std::vector<int>* ends) {
    const int b = c->land_cur;
    int rc = push_common(c, c->iq_land[b], count, ends);
    (void)hipEventRecord(c->land_ev[b], c->stream);
    c->land_used[b] = true;
    c->land_cur ^= 1;
    return rc;
}
int flush_pending(sdrpp_ctx* c) { return flush_pending_opt(c, 1); }
int flush_pending_opt(sdrpp_ctx* c, int drain) {
    if (c->pipelined && c->held.kind >= 0) {  // pushes held for a launch group: the group goes out as it stands (what the host "knows" about the last push needs its plan)
        int rc = tick_group_launch(c);
        if (rc) { return rc; }
    }
    if (drain && c->pipelined && !c->tickq.empty()) {  // pipelined mode: run what the last blocks still have queued
        int rc = tick_drain(c);
        if (rc) { return rc; }
    }
    if (c->pending == 0) { return SDRPP_OK; }
    if (c->async_staged) {  // copy kernels of sdrpp_push_pinned_async still in flight: the pass waits for them on the device
        c->async_staged = false;
        HIPCHK(c, hipEventRecord(c->ev_copy, c->copy_stream));
        HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_copy, 0));
    }
    const int64_t n = c->pending;
    c->pending = 0;  // cleared first: push_common's own helpers may call observing functions
    std::vector<int> ends;
    ends.swap(c->pend_ends);
    return landing_process(c, n, &ends);
}
static int push_args_ok(sdrpp_ctx* c, const void* p, int64_t count) {
    if (!c) { return SDRPP_ERR_INVALID; }
    if ((!p && count > 0) || count < 0 || count > c->max_push) { return fail(c, SDRPP_ERR_INVALID, "push of %lld samples (max %lld)", (long long)count, (long long)c->max_push); }
    if (c->deferred && c->pending + count > c->max_push) {
        return fail(c, SDRPP_ERR_INVALID, "deferred pushes hold %lld samples, %lld more exceed max_push %lld: observe the results first", (long long)c->pending, (long long)count, (long long)c->max_push);
    }
    return SDRPP_OK;
}

// The staging slot of the next block handed to the HOST to fill (pipelined mode): what tick_hold's memcpy does, in the caller's hands.  With
// several blocks per launch (sdrpp_set_pipeline_group) the slot is the launch group's: the block lands behind the ones already held.
int sdrpp_push_stage(sdrpp_ctx* c, int64_t count, float** slot) {
    DeviceScope dev_scope_(c);
    if (!c || !slot) { return SDRPP_ERR_INVALID; }
    if (!c->pipelined) { return fail(c, SDRPP_ERR_INVALID, "sdrpp_push_stage: the context is not in pipelined mode"); }
    if (count <= 0 || count > c->max_push) { return fail(c, SDRPP_ERR_INVALID, "sdrpp_push_stage: count %lld out of range (max_push %lld)", (long long)count, (long long)c->max_push); }
    sdrpp_ctx::Held& H = c->held;
    if (H.kind >= 0 && !H.ends.empty()) {
        const bool fits = H.kind == 1 && (int)H.ends.size() < c->group_max && H.total + count <= c->max_push && group_eligible(c);
        if (!fits) {
            int rc = tick_group_launch(c);
            if (rc) { return rc; }
        }
    }
    if (H.kind != 1) {  // open a group with a fresh slot
        H = sdrpp_ctx::Held{};
        const int si = c->stage_cur;
        if (!c->stage_host[si]) {
            if (hipHostMalloc((void**)&c->stage_host[si], (size_t)c->max_push * 8 + 64, hipHostMallocMapped) != hipSuccess) { return fail(c, SDRPP_ERR_NOMEM, "page-locked staging buffer"); }
        }
        c->stage_cur = (c->stage_cur + 1) % kStageSlots;
        if (c->stage_tick[si]) { tick_wait_done(c, c->stage_tick[si]); }  // its last landing copy has run
        H.kind = 1;
        H.stage_slot = si;
    }
    c->stage_open = H.stage_slot;
    *slot = reinterpret_cast<float*>(c->stage_host[H.stage_slot]) + (size_t)2 * (size_t)H.total;
    return SDRPP_OK;
}
static int push_staged_impl(sdrpp_ctx* c, int64_t count, const volatile uint32_t* pending) {
    if (!c->pipelined || c->stage_open < 0 || c->held.kind != 1 || c->held.stage_slot != c->stage_open) { return fail(c, SDRPP_ERR_INVALID, "sdrpp_push_staged without an open staging slot (sdrpp_push_stage)"); }
    if (count <= 0 || count > c->max_push) { return fail(c, SDRPP_ERR_INVALID, "sdrpp_push_staged: count out of range"); }
    c->stage_open = -1;
    return tick_hold(c, 1, nullptr, count, pending);
}
int sdrpp_push_staged(sdrpp_ctx* c, int64_t count) {
    DeviceScope dev_scope_(c);
    if (!c) { return SDRPP_ERR_INVALID; }
    return push_staged_impl(c, count, nullptr);
}
int sdrpp_push_staged_when(sdrpp_ctx* c, int64_t count, const volatile uint32_t* pending) {
    DeviceScope dev_scope_(c);
    if (!c) { return SDRPP_ERR_INVALID; }
    return push_staged_impl(c, count, pending);  // (a failed plan returns without having waited: the caller joins its own threads)
}

int sdrpp_push(sdrpp_ctx* c, const float* iq_host, int64_t count) {
    DeviceScope dev_scope_(c);
    int rc = push_args_ok(c, iq_host, count);
    if (rc) { return rc; }
    if (c->pipelined) { return tick_hold(c, 1, iq_host, count, nullptr); }
    if (count == 0) { return c->deferred ? SDRPP_OK : push_common(c, nullptr, 0); }
    rc = landing_acquire(c, false);
    if (rc) { return rc; }
    float* land = c->iq_land[c->land_cur] + 2 * c->pending;
    HIPCHK(c, hipMemcpyAsync(land, iq_host, (size_t)count * 2 * sizeof(float), hipMemcpyHostToDevice, c->copy_stream));
    // from here on the copy may be reading the caller's buffer: no return before the host has waited for it
    if (hipEventRecord(c->ev_copy, c->copy_stream) != hipSuccess) {
        (void)hipStreamSynchronize(c->copy_stream);
        return fail(c, SDRPP_ERR_HIP, "hipEventRecord after the landing copy");
    }
    if (c->deferred) {
        HIPCHK(c, hipEventSynchronize(c->ev_copy));  // the caller's buffer is free again; the kernels of the previous pass keep running meanwhile
        c->pending += count;
        c->pend_ends.push_back((int)c->pending);
        return SDRPP_OK;
    }
    // the pass is enqueued behind the copy ON THE DEVICE while the copy runs (planning + launches take longer than the copy of a
    // reference-sized block), and only then does the host wait for the copy: the caller's buffer is free on return, as before
    if (hipStreamWaitEvent(c->stream, c->ev_copy, 0) != hipSuccess) {
        (void)hipEventSynchronize(c->ev_copy);
        return fail(c, SDRPP_ERR_HIP, "hipStreamWaitEvent on the landing copy");
    }
    rc = landing_process(c, count, nullptr);
    HIPCHK(c, hipEventSynchronize(c->ev_copy));
    return rc;
}

// Staging without a host wait: a copy KERNEL on the copy stream reads the page-locked (device-mapped) buffer over the bus; the pass that
// follows waits for it on the device.  (hipMemcpyAsync is not used: see arena_commit.)
__global__ __launch_bounds__(256) void pinned_stage_kernel(const float2* __restrict__ src, float2* __restrict__ dst, long long n) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) { dst[i] = src[i]; }
}
int sdrpp_push_pinned_async(sdrpp_ctx* c, const float* iq_pinned, int64_t count) {
    DeviceScope dev_scope_(c);
    if (!c) { return SDRPP_ERR_INVALID; }
    void* dptr = nullptr;
    if (c->pipelined) {  // the tick's landing role fetches the block from the page-locked buffer itself; sdrpp_push_wait says when it has
        int prc = push_args_ok(c, iq_pinned, count);
        if (prc) { return prc; }
        if (count == 0) { return SDRPP_OK; }
        if (hipHostGetDevicePointer(&dptr, (void*)iq_pinned, 0) != hipSuccess || !dptr) {
            (void)hipGetLastError();
            return tick_hold(c, 1, iq_pinned, count, nullptr);
        }
        return tick_hold(c, 3, iq_pinned, count, nullptr);
    }
    if (!c->deferred || count <= 0 || !iq_pinned || hipHostGetDevicePointer(&dptr, (void*)iq_pinned, 0) != hipSuccess || !dptr) {
        (void)hipGetLastError();
        return sdrpp_push(c, iq_pinned, count);
    }
    int rc = push_args_ok(c, iq_pinned, count);
    if (rc) { return rc; }
    rc = landing_acquire(c, false);
    if (rc) { return rc; }
    float* land = c->iq_land[c->land_cur] + 2 * c->pending;
    hipLaunchKernelGGL(pinned_stage_kernel, dim3((unsigned)std::max<int64_t>(1, std::min<int64_t>((count + 1023) / 1024, 128))), dim3(256), 0, c->copy_stream, (const float2*)dptr, (float2*)land,
                       (long long)count);
    c->async_staged = true;
    c->async_inflight = true;
    c->pending += count;
    c->pend_ends.push_back((int)c->pending);
    return SDRPP_OK;
}

int sdrpp_push_wait(sdrpp_ctx* c) {
    DeviceScope dev_scope_(c);
    if (!c) { return SDRPP_ERR_INVALID; }
    if (c->pipelined) {  // every landing copy so far has run once its tick is complete (what is still held goes out first)
        int rc = tick_group_launch(c);
        if (rc) { return rc; }
        if (c->land_tick) { tick_wait_done(c, c->land_tick); }
        return SDRPP_OK;
    }
    // (not `async_staged`: a flushing call that does not host-synchronise — sdrpp_fft_lines, sdrpp_vfo_out_count, a setter — clears that
    // one while the copy kernels may still be reading the caller's page-locked buffers)
    if (c->async_inflight) {
        HIPCHK(c, hipStreamSynchronize(c->copy_stream));
        c->async_inflight = false;
    }
    return SDRPP_OK;
}

int sdrpp_push_device(sdrpp_ctx* c, const float* iq_dev, int64_t count) {
    DeviceScope dev_scope_(c);
    int rc = push_args_ok(c, iq_dev, count);
    if (rc) { return rc; }
    if (c->pipelined) { return tick_hold(c, 0, iq_dev, count, nullptr); }  // read in place, one tick from now at the earliest
    if (!c->deferred) { return push_common(c, iq_dev, count); }  // read in place
    if (count == 0) { return SDRPP_OK; }
    rc = landing_acquire(c, false);
    if (rc) { return rc; }
    HIPCHK(c, hipMemcpyAsync(c->iq_land[c->land_cur] + 2 * c->pending, iq_dev, (size_t)count * 2 * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
    c->pending += count;
    c->pend_ends.push_back((int)c->pending);
    return SDRPP_OK;
}

// ---- raw wire formats (ingest_kernels.h) ----
// One routine behind sdrpp_push_raw, sdrpp_push_int16 and sdrpp_push_frame; `fmt` has been checked.
static int push_raw_impl(sdrpp_ctx* c, const void* iq_host, int64_t count, const sdrpp_iq_format& fmt) {
    int rc = push_args_ok(c, iq_host, count);
    if (rc) { return rc; }
    if (c->pipelined) { return tick_hold(c, 2, iq_host, count, nullptr, &fmt); }
    if (count == 0) { return c->deferred ? SDRPP_OK : push_common(c, nullptr, 0); }
    rc = landing_acquire(c, true);
    if (rc) { return rc; }
    const int b = c->land_cur;
    // (4 bytes per staged sample whatever the format: the pushes of a deferred pass may differ in theirs, and the conversion of one must not find the
    // raw bytes of the next where it still reads)
    char* raw = reinterpret_cast<char*>(c->iq_land16[b]) + (size_t)4 * (size_t)c->pending;
    const size_t bytes = (size_t)count * iq_format_bytes(fmt.type);
    HIPCHK(c, hipMemcpyAsync(raw, iq_host, bytes, hipMemcpyHostToDevice, c->copy_stream));
    HIPCHK(c, hipEventRecord(c->ev_copy, c->copy_stream));
    HIPCHK(c, hipEventSynchronize(c->ev_copy));
    if (fmt.type == SDRPP_IQ_U8 && (c->u8_tab.size() != 256 || memcmp(c->u8_tab.data(), fmt.table, 256 * sizeof(float)) != 0)) {
        if (!c->d_u8_tab) {
            rc = dev_alloc(c, &c->d_u8_tab, 256);
            if (rc) { return rc; }
        }
        c->u8_tab.assign(fmt.table, fmt.table + 256);
        // on the stream of the conversions: behind those that still read the previous table
        if (hipMemcpyAsync(c->d_u8_tab, c->u8_tab.data(), 256 * sizeof(float), hipMemcpyHostToDevice, c->launch_stream) != hipSuccess) {
            c->u8_tab.clear();
            return fail(c, SDRPP_ERR_HIP, "upload of the U8 table failed");
        }
    }
    {
        FamilyTimer t(c, F_MISC);
        const long long n16 = (long long)(bytes / 16);
        launch(c, ingest_kernel, dim3((unsigned)std::max<long long>(1, std::min<long long>((n16 + 255) / 256, 2048))), dim3(256), 0, (const void*)raw, c->iq_land[b] + 2 * c->pending, (long long)bytes, fmt.type,
               fmt.type == SDRPP_IQ_U8 ? 0.0f : 1.0f / fmt.scalar, (const float*)c->d_u8_tab);
    }
    if (c->deferred) {
        c->pending += count;
        c->pend_ends.push_back((int)c->pending);
        return SDRPP_OK;
    }
    return landing_process(c, count, nullptr);
}
int sdrpp_push_int16(sdrpp_ctx* c, const int16_t* iq_host, int64_t count) {
    DeviceScope dev_scope_(c);
    if (!c) { return SDRPP_ERR_INVALID; }
    return push_raw_impl(c, iq_host, count, sdrpp_iq_format{ SDRPP_IQ_I16, 32768.0f, nullptr });  // (x * (1.0f / 32768.0f) is exact: what x / 32768 gave)
}
int sdrpp_push_raw(sdrpp_ctx* c, const void* iq_host, int64_t count, const sdrpp_iq_format* fmt) {
    DeviceScope dev_scope_(c);
    if (!c) { return SDRPP_ERR_INVALID; }
    if (!fmt) { return fail(c, SDRPP_ERR_INVALID, "sdrpp_push_raw: no format"); }
    if (fmt->type == SDRPP_IQ_I8 || fmt->type == SDRPP_IQ_I16) {
        if (!std::isfinite(fmt->scalar) || fmt->scalar == 0.0f) { return fail(c, SDRPP_ERR_INVALID, "sdrpp_push_raw: scalar %g (need a finite number other than 0)", (double)fmt->scalar); }
    }
    else if (fmt->type == SDRPP_IQ_U8) {
        if (!fmt->table) { return fail(c, SDRPP_ERR_INVALID, "sdrpp_push_raw: SDRPP_IQ_U8 needs a table (sdrpp_design_u8_table)"); }
    }
    else { return fail(c, SDRPP_ERR_INVALID, "sdrpp_push_raw: unknown format %d", fmt->type); }
    return push_raw_impl(c, iq_host, count, *fmt);
}
int sdrpp_push_frame(sdrpp_ctx* c, const unsigned char* frame, int bytes, int* samples) {
    DeviceScope dev_scope_(c);
    if (!c) { return SDRPP_ERR_INVALID; }
    if (samples) { *samples = 0; }
    if (!frame || bytes < 8) { return fail(c, SDRPP_ERR_INVALID, "sdrpp_push_frame: %d bytes (a frame has an 8-byte header)", bytes); }
    // SampleStreamDecompressor::process (sample_stream_decompressor.h:13-34); PCMType (pcm_type.h): 0 I8, 1 I16, 2 F32
    uint16_t type;
    float scaler;
    memcpy(&type, frame + 2, sizeof(type));
    memcpy(&scaler, frame + 4, sizeof(scaler));
    const unsigned char* data = frame + 8;
    int n = 0, rc = SDRPP_OK;
    if (type == 2) {
        n = (bytes - 8) / 8;
        if (n > 0) {
            // (the data start 8 bytes into the caller's frame: whatever alignment that has, the push copies bytes)
            rc = sdrpp_push(c, reinterpret_cast<const float*>(data), n);
        }
    }
    else if (type == 1 || type == 0) {
        n = (bytes - 8) / (type == 1 ? 4 : 2);
        if (n > 0) {
            sdrpp_iq_format fmt{ type == 1 ? SDRPP_IQ_I16 : SDRPP_IQ_I8, (type == 1 ? 32768.0f : 128.0f) / scaler, nullptr };
            rc = sdrpp_push_raw(c, data, n, &fmt);
        }
    }
    if (!rc && samples) { *samples = n; }
    return rc;
}
int sdrpp_abi_sizeof_iq_format(void) { return (int)sizeof(sdrpp_iq_format); }

// page-locked host memory for buffers the caller pushes from (an H2D copy from pageable memory is staged by the runtime: ~3x slower)
void* sdrpp_host_alloc(size_t bytes) {
    void* p = nullptr;
    if (hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocDefault) != hipSuccess) { return nullptr; }
    return p;
}
void sdrpp_host_free(void* p) {
    if (p) { (void)hipHostFree(p); }
}
void* sdrpp_device_alloc(sdrpp_ctx* c, size_t bytes) {
    if (!c) { return nullptr; }
    DeviceScope dev_scope_(c);
    void* p = nullptr;
    if (hipMalloc(&p, bytes ? bytes : 16) != hipSuccess) { return nullptr; }
    return p;
}
void sdrpp_device_free(sdrpp_ctx* c, void* p) {
    if (!c || !p) { return; }
    DeviceScope dev_scope_(c);
    (void)hipFree(p);
}
// THREAD-SAFE, unlike the rest of a context: a several-GPU host copies a front end's newest line from its gather thread while the worker thread
// is inside sdrpp_push / sdrpp_result_wait on the same context (host/sdrpp_gpu_blocks.h: copyLatestLineDevice).  So the call touches nothing of
// the context that ever changes: a stream of its own (created with the context), its own lock, no error text (the code is all the caller gets).
// It is therefore NOT ordered with the work on the context's stream — it is for buffers whose content is complete (written by an earlier
// sdrpp_device_copy, or by sdrpp_fft_copy_device followed by sdrpp_sync) and it does not wait for the launches queued there.
int sdrpp_device_copy(sdrpp_ctx* c, void* dst, const void* src, size_t bytes, int kind) {
    if (!c) { return SDRPP_ERR_INVALID; }
    if (kind < 0 || kind > 2 || (bytes && (!dst || !src))) { return SDRPP_ERR_INVALID; }
    if (!bytes) { return SDRPP_OK; }
    DeviceScope dev_scope_(c);
    const hipMemcpyKind k = kind == 0 ? hipMemcpyHostToDevice : (kind == 1 ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost);
    std::lock_guard<std::mutex> lck(c->side_mtx);
    if (hipMemcpyAsync(dst, src, bytes, k, c->side_stream) != hipSuccess) { return SDRPP_ERR_HIP; }
    if (hipStreamSynchronize(c->side_stream) != hipSuccess) { return SDRPP_ERR_HIP; }
    return SDRPP_OK;
}

int sdrpp_set_deferred(sdrpp_ctx* c, int on) {
    DeviceScope dev_scope_(c);
    if (!c) { return SDRPP_ERR_INVALID; }
    if (on && c->pipelined) { return fail(c, SDRPP_ERR_INVALID, "deferred and pipelined processing exclude each other"); }
    int rc = flush_pending(c);
    c->deferred = on != 0;
    return rc;
}
int64_t sdrpp_pending(sdrpp_ctx* c) { return c ? c->pending : SDRPP_ERR_INVALID; }

// ---- pipelined execution ----------------------------------------------------------------------------------------------------------------
int sdrpp_set_pipelined(sdrpp_ctx* c, int on, int result_flags) {
    DeviceScope dev_scope_(c);
    if (!c || result_flags < 0 || result_flags > 31) { return SDRPP_ERR_INVALID; }
    if (on && c->deferred) { return fail(c, SDRPP_ERR_INVALID, "deferred and pipelined processing exclude each other"); }
    int rc = flush_pending(c);  // (drains the queue when the mode is being left)
    if (rc) { return rc; }
    for (auto& R : c->res) {
        if (R.held) { return fail(c, SDRPP_ERR_INVALID, "results of block %llu are still held", (unsigned long long)R.ticket); }
    }
    c->held = sdrpp_ctx::Held{};
    c->stage_open = -1;
    c->pipelined = on != 0;
    c->res_flags = on ? result_flags : 0;
    c->res_qpsk_soft = false;
    return SDRPP_OK;
}
int sdrpp_set_pipeline_group(sdrpp_ctx* c, int max_blocks, int adaptive) {
    DeviceScope dev_scope_(c);
    if (!c || max_blocks < 1 || max_blocks > kGroupMax) { return c ? fail(c, SDRPP_ERR_INVALID, "sdrpp_set_pipeline_group: 1 .. %d blocks per launch", kGroupMax) : SDRPP_ERR_INVALID; }
    if (c->pipelined) {
        int rc = tick_group_launch(c);  // what is held goes out under the old rule
        if (rc) { return rc; }
    }
    c->group_max = max_blocks;
    c->group_adaptive = (adaptive & 1) != 0;
    c->stage_pend_stable = (adaptive & 2) != 0;
    return SDRPP_OK;
}
int sdrpp_pipeline_launch_held(sdrpp_ctx* c) {
    DeviceScope dev_scope_(c);
    if (!c) { return SDRPP_ERR_INVALID; }
    return c->pipelined ? tick_group_launch(c) : SDRPP_OK;
}
int sdrpp_pipeline_group_stats(sdrpp_ctx* c, int64_t* out, int max) {
    if (!c || !out || max < 0) { return SDRPP_ERR_INVALID; }
    const int64_t v[5] = { (int64_t)c->groups, c->stat_groups, c->stat_group_blocks, c->stat_group_max, (int64_t)c->held.ends.size() };
    int n = 0;
    for (; n < 5 && n < max; n++) { out[n] = v[n]; }
    return n;
}
uint64_t sdrpp_ticket(sdrpp_ctx* c) { return c ? c->pushes : 0; }
int sdrpp_pipeline_flush(sdrpp_ctx* c) {
    DeviceScope dev_scope_(c);
    if (!c) { return SDRPP_ERR_INVALID; }
    if (!c->pipelined) { return SDRPP_OK; }
    int rc = tick_group_launch(c);
    return rc ? rc : tick_drain(c);
}
static bool ticket_is_held_back(const sdrpp_ctx* c, uint64_t ticket) {  // pushed, but its launch group has not gone out yet
    return c->held.kind >= 0 && !c->held.ends.empty() && ticket <= c->pushes && ticket + c->held.ends.size() > c->pushes;
}
static sdrpp_ctx::Result* result_of(sdrpp_ctx* c, uint64_t ticket) {
    if (!c || ticket == 0 || ticket > c->pushes) { return nullptr; }
    sdrpp_ctx::Result& R = c->res[ticket % kResMeta];
    if (R.ticket != ticket) { return nullptr; }
    if (R.held) { return &R; }  // (its bytes are where the host was told, whatever has happened to the ring since)
    return (R.epoch == c->res_epoch && tick_results_region(c, R.group)) ? &R : nullptr;  // (the ring has not come round to its group's region)
}
int sdrpp_result_ready(sdrpp_ctx* c, uint64_t ticket) {
    if (c && ticket_is_held_back(c, ticket)) { return 0; }
    sdrpp_ctx::Result* R = result_of(c, ticket);
    if (!R) { return c ? fail(c, SDRPP_ERR_NOT_FOUND, "no results for block %llu (not gathered, overwritten, or processed as an ordinary pass)", (unsigned long long)ticket) : SDRPP_ERR_INVALID; }
    if (R->done_tick > c->ticks) { return 0; }
    DeviceScope dev_scope_(c);
    return tick_results_visible(c, R->done_tick, false);
}
int sdrpp_result_wait(sdrpp_ctx* c, uint64_t ticket, sdrpp_result* out) {
    DeviceScope dev_scope_(c);
    if (!c || !out) { return SDRPP_ERR_INVALID; }
    if (ticket_is_held_back(c, ticket)) {  // nothing more is coming for its group: it goes out as it stands
        int rc = tick_group_launch(c);
        if (rc) { return rc; }
    }
    sdrpp_ctx::Result* R = result_of(c, ticket);
    if (!R) { return fail(c, SDRPP_ERR_NOT_FOUND, "no results for block %llu (not gathered, overwritten, or processed as an ordinary pass)", (unsigned long long)ticket); }
    while (R->done_tick > c->ticks) {  // its last levels have not been launched yet: nothing more is coming, run them without new input
        int rc = tick_group_launch(c);  // (younger pushes held for a group ride along: their first level shares the launch)
        if (!rc && R->done_tick <= c->ticks) { break; }
        if (!rc) { rc = arena_begin(c); }
        if (!rc) { rc = tick_launch(c, nullptr); }
        if (rc) { return rc; }
        if (c->tickq.empty() && R->done_tick > c->ticks) { return fail(c, SDRPP_ERR_HIP, "internal: block %llu cannot complete", (unsigned long long)ticket); }
    }
    {   // complete on the device AND visible here (the flag alone is not: see tick_results_visible)
        const int vis = tick_results_visible(c, R->done_tick, true);
        if (vis < 0) { return vis; }
    }
    if (!tick_is_done(c, R->done_tick)) { return fail(c, SDRPP_ERR_HIP, "tick %llu did not complete", (unsigned long long)R->done_tick); }
    if (!R->held) {
        sdrpp_ctx::ResRegion* g = tick_results_region(c, R->group);
        if (!g) { return fail(c, SDRPP_ERR_NOT_FOUND, "no results for block %llu (overwritten)", (unsigned long long)ticket); }
        R->held = true;
        g->held++;
    }
    const char* base = R->base;
    out->ticket = ticket;
    out->n_vfo = (int)R->ids.size();
    out->ids = R->ids.data();
    out->offsets = R->offsets.data();
    out->counts = R->counts.data();
    out->samples = reinterpret_cast<const float*>(base);
    out->n_lines = R->n_lines;
    // shapes and presence as the block was planned: sdrpp_fft_set_view / sdrpp_fft_configure between push and wait do not re-label the slot
    out->fft_size = R->fft_size;
    out->data_width = R->data_width;
    const bool zo = R->n_lines > 0 && (R->flags & 2) && R->data_width > 0;
    out->zoomed = zo ? reinterpret_cast<const float*>(base + R->off_zoomed) : nullptr;
    out->index = zo ? reinterpret_cast<const int32_t*>(base + R->off_index) : nullptr;
    out->raw = (R->n_lines > 0 && (R->flags & 4)) ? reinterpret_cast<const float*>(base + R->off_raw) : nullptr;
    out->n_iq = R->n_iq;
    out->iq = R->n_iq > 0 ? reinterpret_cast<const float*>(base + R->off_iq) : nullptr;
    return SDRPP_OK;
}
int sdrpp_result_rec(sdrpp_ctx* c, uint64_t ticket, int id, const void** data, sdrpp_rec_info* info) {
    if (!c) { return SDRPP_ERR_INVALID; }
    sdrpp_ctx::Result* R = result_of(c, ticket);
    if (!R || !R->held) { return fail(c, SDRPP_ERR_INVALID, "sdrpp_result_rec: block %llu is not held (between sdrpp_result_wait and sdrpp_result_release)", (unsigned long long)ticket); }
    for (size_t i = 0; i < R->rec_ids.size(); i++) {
        if (R->rec_ids[i] != id) { continue; }
        if (data) { *data = R->base + R->rec_off[i]; }
        if (info) { memcpy(info, R->base + R->rec_info_off[i], sizeof(sdrpp_rec_info)); }
        return SDRPP_OK;
    }
    return fail(c, SDRPP_ERR_NOT_FOUND, "block %llu holds nothing of a recorder sink of VFO %d", (unsigned long long)ticket, id);
}
int sdrpp_pipeline_set_rds_results(sdrpp_ctx* c, int on) {
    DeviceScope dev_scope_(c);
    if (!c) { return SDRPP_ERR_INVALID; }
    if (!c->pipelined) { return fail(c, SDRPP_ERR_INVALID, "sdrpp_pipeline_set_rds_results outside pipelined mode"); }
    FLUSH_PENDING(c);
    c->res_flags = on ? (c->res_flags | SDRPP_RESULT_RDS) : (c->res_flags & ~SDRPP_RESULT_RDS);
    return SDRPP_OK;
}
int sdrpp_result_rds(sdrpp_ctx* c, uint64_t ticket, int id, const float** data, int* count) {
    if (!c) { return SDRPP_ERR_INVALID; }
    sdrpp_ctx::Result* R = result_of(c, ticket);
    if (!R || !R->held) { return fail(c, SDRPP_ERR_INVALID, "sdrpp_result_rds: block %llu is not held (between sdrpp_result_wait and sdrpp_result_release)", (unsigned long long)ticket); }
    for (size_t i = 0; i < R->rds_ids.size(); i++) {
        if (R->rds_ids[i] != id) { continue; }
        if (data) { *data = reinterpret_cast<const float*>(R->base + R->rds_off[i]); }
        if (count) { *count = R->rds_counts[i]; }
        return SDRPP_OK;
    }
    return fail(c, SDRPP_ERR_NOT_FOUND, "block %llu holds nothing of an RDS branch of VFO %d", (unsigned long long)ticket, id);
}
int sdrpp_pipeline_set_sym_results(sdrpp_ctx* c, int on) {
    DeviceScope dev_scope_(c);
    if (!c) { return SDRPP_ERR_INVALID; }
    if (!c->pipelined) { return fail(c, SDRPP_ERR_INVALID, "sdrpp_pipeline_set_sym_results outside pipelined mode"); }
    FLUSH_PENDING(c);
    c->res_flags = on ? (c->res_flags | SDRPP_RESULT_SYM) : (c->res_flags & ~SDRPP_RESULT_SYM);
    return SDRPP_OK;
}
// (the counts are the loop's own result: they lie in the slot, complete since sdrpp_result_wait returned for this block)
int sdrpp_result_sym(sdrpp_ctx* c, uint64_t ticket, int id, const float** soft, const uint8_t** bits, int* count) {
    if (!c) { return SDRPP_ERR_INVALID; }
    sdrpp_ctx::Result* R = result_of(c, ticket);
    if (!R || !R->held) { return fail(c, SDRPP_ERR_INVALID, "sdrpp_result_sym: block %llu is not held (between sdrpp_result_wait and sdrpp_result_release)", (unsigned long long)ticket); }
    for (size_t i = 0; i < R->sym_ids.size(); i++) {
        if (R->sym_ids[i] != id) { continue; }
        int cnt[kGroupMax] = {};
        const int j = std::min(R->sym_push[i], kGroupMax - 1);
        memcpy(cnt, R->base + R->sym_cnt_off[i], (size_t)(j + 1) * sizeof(int));
        size_t lo = 0;
        for (int q = 0; q < j; q++) { lo += (size_t)std::max(cnt[q], 0); }
        if (soft) { *soft = reinterpret_cast<const float*>(R->base + R->sym_soft_off[i]) + lo; }
        if (bits) { *bits = reinterpret_cast<const uint8_t*>(R->base + R->sym_bits_off[i]) + lo; }
        if (count) { *count = cnt[j]; }
        return SDRPP_OK;
    }
    return fail(c, SDRPP_ERR_NOT_FOUND, "block %llu holds nothing of a symbol branch of VFO %d", (unsigned long long)ticket, id);
}
int sdrpp_pipeline_set_rds_bits_results(sdrpp_ctx* c, int on) {
    DeviceScope dev_scope_(c);
    if (!c) { return SDRPP_ERR_INVALID; }
    if (!c->pipelined) { return fail(c, SDRPP_ERR_INVALID, "sdrpp_pipeline_set_rds_bits_results outside pipelined mode"); }
    FLUSH_PENDING(c);
    c->res_flags = on ? (c->res_flags | SDRPP_RESULT_RDS_BITS) : (c->res_flags & ~SDRPP_RESULT_RDS_BITS);
    return SDRPP_OK;
}
// (the counts are the job's own result: they lie in the slot, complete since sdrpp_result_wait returned for this block)
int sdrpp_result_rds_bits(sdrpp_ctx* c, uint64_t ticket, int id, const float** soft, const uint8_t** bits, int* count) {
    if (!c) { return SDRPP_ERR_INVALID; }
    sdrpp_ctx::Result* R = result_of(c, ticket);
    if (!R || !R->held) { return fail(c, SDRPP_ERR_INVALID, "sdrpp_result_rds_bits: block %llu is not held (between sdrpp_result_wait and sdrpp_result_release)", (unsigned long long)ticket); }
    for (size_t i = 0; i < R->rdsd_ids.size(); i++) {
        if (R->rdsd_ids[i] != id) { continue; }
        int cnt[kGroupMax] = {};
        const int j = std::min(R->rdsd_push[i], kGroupMax - 1);
        memcpy(cnt, R->base + R->rdsd_cnt_off[i], (size_t)(j + 1) * sizeof(int));
        size_t lo = 0;
        for (int q = 0; q < j; q++) { lo += (size_t)std::max(cnt[q], 0); }
        if (soft) { *soft = reinterpret_cast<const float*>(R->base + R->rdsd_soft_off[i]) + lo; }
        if (bits) { *bits = reinterpret_cast<const uint8_t*>(R->base + R->rdsd_bits_off[i]) + lo; }
        if (count) { *count = cnt[j]; }
        return SDRPP_OK;
    }
    return fail(c, SDRPP_ERR_NOT_FOUND, "block %llu holds nothing of an RDS demodulator of VFO %d", (unsigned long long)ticket, id);
}
int sdrpp_pipeline_set_qpsk_results(sdrpp_ctx* c, int on, int with_soft) {
    DeviceScope dev_scope_(c);
    if (!c) { return SDRPP_ERR_INVALID; }
    if (!c->pipelined) { return fail(c, SDRPP_ERR_INVALID, "sdrpp_pipeline_set_qpsk_results outside pipelined mode"); }
    FLUSH_PENDING(c);
    c->res_flags = on ? (c->res_flags | SDRPP_RESULT_QPSK) : (c->res_flags & ~SDRPP_RESULT_QPSK);
    c->res_qpsk_soft = on && with_soft;
    return SDRPP_OK;
}
// (the counts are the job's own result: they lie in the slot, complete since sdrpp_result_wait returned for this block)
int sdrpp_result_qpsk(sdrpp_ctx* c, uint64_t ticket, int id, const float** soft_iq, const int8_t** packed, int* count) {
    if (!c) { return SDRPP_ERR_INVALID; }
    sdrpp_ctx::Result* R = result_of(c, ticket);
    if (!R || !R->held) { return fail(c, SDRPP_ERR_INVALID, "sdrpp_result_qpsk: block %llu is not held (between sdrpp_result_wait and sdrpp_result_release)", (unsigned long long)ticket); }
    for (size_t i = 0; i < R->qpsk_ids.size(); i++) {
        if (R->qpsk_ids[i] != id) { continue; }
        int cnt[kGroupMax] = {};
        const int j = std::min(R->qpsk_push[i], kGroupMax - 1);
        memcpy(cnt, R->base + R->qpsk_cnt_off[i], (size_t)(j + 1) * sizeof(int));
        size_t lo = 0;
        for (int q = 0; q < j; q++) { lo += (size_t)std::max(cnt[q], 0); }
        if (soft_iq) { *soft_iq = (R->qpsk_soft_off[i] == SIZE_MAX) ? nullptr : reinterpret_cast<const float*>(R->base + R->qpsk_soft_off[i]) + 2 * lo; }  // (NULL: the float pairs were not asked for)
        if (packed) { *packed = reinterpret_cast<const int8_t*>(R->base + R->qpsk_packed_off[i]) + 2 * lo; }
        if (count) { *count = cnt[j]; }
        return SDRPP_OK;
    }
    return fail(c, SDRPP_ERR_NOT_FOUND, "block %llu holds nothing of a QPSK demodulator of VFO %d", (unsigned long long)ticket, id);
}
int sdrpp_pipeline_set_frame_results(sdrpp_ctx* c, int on) {
    DeviceScope dev_scope_(c);
    if (!c) { return SDRPP_ERR_INVALID; }
    if (!c->pipelined) { return fail(c, SDRPP_ERR_INVALID, "sdrpp_pipeline_set_frame_results outside pipelined mode"); }
    FLUSH_PENDING(c);
    c->res_flags = on ? (c->res_flags | SDRPP_RESULT_FRAMES) : (c->res_flags & ~SDRPP_RESULT_FRAMES);
    return SDRPP_OK;
}
// (the counts are the job's own result: they lie in the slot, complete since sdrpp_result_wait returned for this block)
int sdrpp_result_frames(sdrpp_ctx* c, uint64_t ticket, int id, const uint8_t** records, int* count) {
    if (!c) { return SDRPP_ERR_INVALID; }
    sdrpp_ctx::Result* R = result_of(c, ticket);
    if (!R || !R->held) { return fail(c, SDRPP_ERR_INVALID, "sdrpp_result_frames: block %llu is not held (between sdrpp_result_wait and sdrpp_result_release)", (unsigned long long)ticket); }
    for (size_t i = 0; i < R->frame_ids.size(); i++) {
        if (R->frame_ids[i] != id) { continue; }
        int cnt[kGroupMax] = {};
        const int j = std::min(R->frame_push[i], kGroupMax - 1);
        memcpy(cnt, R->base + R->frame_cnt_off[i], (size_t)(j + 1) * sizeof(int));
        size_t lo = 0;
        for (int q = 0; q < j; q++) { lo += (size_t)std::max(cnt[q], 0); }
        if (records) { *records = reinterpret_cast<const uint8_t*>(R->base + R->frame_rec_off[i]) + lo * (size_t)R->frame_stride[i]; }
        if (count) { *count = std::max(cnt[j], 0); }
        return SDRPP_OK;
    }
    return fail(c, SDRPP_ERR_NOT_FOUND, "block %llu holds nothing of a framer of VFO %d", (unsigned long long)ticket, id);
}
int sdrpp_result_meters(sdrpp_ctx* c, uint64_t ticket, const float** data, int* n_lines, int* n_meters) {
    if (!c) { return SDRPP_ERR_INVALID; }
    sdrpp_ctx::Result* R = result_of(c, ticket);
    if (!R || !R->held) { return fail(c, SDRPP_ERR_INVALID, "sdrpp_result_meters: block %llu is not held (between sdrpp_result_wait and sdrpp_result_release)", (unsigned long long)ticket); }
    if (R->n_meters < 0) { return fail(c, SDRPP_ERR_NOT_FOUND, "block %llu was pushed without a table of signal meters", (unsigned long long)ticket); }
    if (data) { *data = R->n_lines > 0 ? reinterpret_cast<const float*>(R->base + R->off_meters) : nullptr; }
    if (n_lines) { *n_lines = R->n_lines; }
    if (n_meters) { *n_meters = R->n_meters; }
    return SDRPP_OK;
}
int sdrpp_result_release(sdrpp_ctx* c, uint64_t ticket) {
    if (!c || ticket == 0 || ticket > c->pushes) { return c ? SDRPP_ERR_NOT_FOUND : SDRPP_ERR_INVALID; }
    sdrpp_ctx::Result& R = c->res[ticket % kResMeta];
    if (R.ticket != ticket) { return SDRPP_ERR_NOT_FOUND; }
    if (R.held) {
        if (sdrpp_ctx::ResRegion* g = tick_results_region(c, R.group)) {
            if (g->held > 0) { g->held--; }
        }
        if (R.epoch != c->res_epoch) {  // a ring the results outgrew while the host held this block: freed with its last held block
            for (size_t i = 0; i < c->res_retired.size(); i++) {
                if (c->res_retired[i].epoch == R.epoch && --c->res_retired[i].held <= 0) {
                    DeviceScope dev_scope_(c);
                    (void)hipHostFree(c->res_retired[i].ring);
                    c->res_retired.erase(c->res_retired.begin() + (long)i);
                    break;
                }
            }
        }
    }
    R.held = false;
    R.ticket = 0;
    return SDRPP_OK;
}

int sdrpp_result_take_lines(sdrpp_ctx* c, uint64_t ticket, float* zoomed_dst, int32_t* index_dst, int max_lines, int* n_lines) {
    sdrpp_result r{};
    int rc = sdrpp_result_wait(c, ticket, &r);
    if (rc) { return rc; }
    if (n_lines) { *n_lines = r.n_lines; }
    if (r.n_lines > max_lines) {
        (void)sdrpp_result_release(c, ticket);
        return fail(c, SDRPP_ERR_INVALID, "block %llu completed %d lines, room for %d", (unsigned long long)ticket, r.n_lines, max_lines);
    }
    if (r.n_lines > 0 && r.zoomed) {
        const size_t bytes = (size_t)r.n_lines * (size_t)r.data_width * 4;
        if (zoomed_dst) { memcpy(zoomed_dst, r.zoomed, bytes); }
        if (index_dst) { memcpy(index_dst, r.index, bytes); }
    }
    return sdrpp_result_release(c, ticket);
}
int sdrpp_pipeline_stats(sdrpp_ctx* c, int64_t* out, int max) {
    if (!c || !out || max < 0) { return SDRPP_ERR_INVALID; }
    const int64_t head[SDRPP_PIPELINE_STATS_HEAD] = { (int64_t)c->ticks, c->stat_tick_blocks, c->stat_pass_blocks, c->stat_crowded, c->stat_last_depth, (int64_t)TR_COUNT, 0, c->stat_last_table_bytes };  // [6]: reserved, always 0
    int n = 0;
    for (; n < SDRPP_PIPELINE_STATS_HEAD && n < max; n++) { out[n] = head[n]; }
    for (int r = 0; r < TR_COUNT && n < max; r++, n++) { out[n] = c->stat_role_wgs[r]; }
    return n;
}
const char* sdrpp_pipeline_role_name(int role) {
    static const char* const names[] = { "none", "copy", "carry", "rot", "fcm_132_4", "fcm_6", "fcm_10", "fcm_16", "fcm16_132_4", "fcl_0", "fcl_pf", "toep_c", "toep_r", "toep_q",
                                         "firb_c", "firb_r", "firb_s", "firb_q", "pre", "seq", "fft_s10", "fft_s11", "fft_s12", "fft_p1_5", "fft_p1_6", "fft_p1_7", "fft_p1_8", "fft_p1_9",
                                         "fft_p1_10", "fft_p2_7", "fft_p2_8", "fft_p2_9", "fft_p2_10", "fft_p2row", "fft_tr", "zoom_16", "zoom_4", "zoom_1", "polyc", "deemp_p0", "deemp_p1",
                                         "dc_p0", "dc_p1", "wf_ring", "wf_trace", "pipe", "rotx16", "fird", "ssbx", "s1_1", "s1d_1", "f2_1", "poly", "ifc" };
    static_assert(sizeof(names) / sizeof(names[0]) == TR_COUNT, "role names out of step with TickRole");
    return (role >= 0 && role < TR_COUNT) ? names[role] : nullptr;
}
int sdrpp_pass_form_stats(sdrpp_ctx* c, int64_t* out, const char** names, int max) {
    static const char* const extra[] = { "polyb_4", "polyb_8", "polyb_4_odd", "polyb_8_odd", "s1_8", "s1_4", "s1_2", "s1d_8", "s1d_4", "s1d_2", "f2_8_44_3", "f2_8", "f2_4", "f2_2", "rotx_1" };
    static_assert(sizeof(extra) / sizeof(extra[0]) == PF_COUNT - TR_COUNT, "form names out of step with PassForm");
    if (max < 0 || (out && !c)) { return SDRPP_ERR_INVALID; }
    int n = 0;
    for (; n < PF_COUNT && n < max; n++) {
        if (out) { out[n] = c->stat_pass_forms[n]; }
        if (names) { names[n] = n < TR_COUNT ? sdrpp_pipeline_role_name(n) : extra[n - TR_COUNT]; }
    }
    return n;
}

// ---- measurement ---------------------------------------------------------------------------------------------------------------------
int sdrpp_timing_enable(sdrpp_ctx* c, int on) {
    DeviceScope dev_scope_(c);
    if (!c) { return SDRPP_ERR_INVALID; }
    timing_flush(c);
    c->timing = on != 0;
    c->timing_mask = (on > 1) ? (unsigned)(on >> 1) : 0xffffffffu;  // on = 1: all families; on = 1 | (mask << 1): selected ones
    for (int i = 0; i < SDRPP_NUM_KERNEL_FAMILIES; i++) {
        c->fam_ms[i] = 0.0;
        c->fam_launch[i] = 0;
    }
    return SDRPP_OK;
}

int sdrpp_timing_read(sdrpp_ctx* c, double* ms, int64_t* launches) {
    DeviceScope dev_scope_(c);
    if (!c) { return SDRPP_ERR_INVALID; }
    timing_flush(c);
    for (int i = 0; i < SDRPP_NUM_KERNEL_FAMILIES; i++) {
        if (ms) { ms[i] = c->fam_ms[i]; }
        if (launches) { launches[i] = c->fam_launch[i]; }
    }
    return SDRPP_OK;
}

}  // extern "C"
