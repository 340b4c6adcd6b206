// AF chain and pre-processing recurrences: the exact DC blocker, de-emphasis and DC blocker as two-level scans, conjugate.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <sdrpp_gfx950.h>
#include "fft_kernels.h"

namespace sdrpp_k {

// The reference's DC blocker recursion itself (dc_blocker.h:54-60: out = in - offset; offset += out * rate, product rounded, then added)
// over the wideband stream, for the parity mode of the pre-processing chain: ONE wavefront walks the block, 64 samples per coalesced
// load, every lane evaluating the same recursion with sample i taken from lane i (v_readlane).  ~40 cycles per sample: a few times real
// time for a 10 MS/s stream — the default (a two-level scan of affine maps, vfo_deemph_kernel<1, *>) is the fast one and agrees to ~5e-5.
__global__ __launch_bounds__(64) void iq_dc_block_exact_kernel(const float2* __restrict__ in, float2* __restrict__ out, int n, float rate, float2* __restrict__ state, int conj) {
    const int lane = (int)threadIdx.x;
    float offr = state->x, offi = state->y;
    for (int base = 0; base < n; base += 64) {
        const int cnt = (n - base < 64) ? n - base : 64;
        const float2 v = (lane < cnt) ? in[base + lane] : make_float2(0.0f, 0.0f);
        float2 res = make_float2(0.0f, 0.0f);
        for (int i = 0; i < cnt; i++) {
            const float xr = wave_bcast(v.x, i), xi = wave_bcast(v.y, i);
            const float orr = xr - offr, oi = xi - offi;
            const float pr = orr * rate, pi = oi * rate;
            offr = offr + pr;
            offi = offi + pi;
            if (lane == i) { res = make_float2(orr, conj ? -oi : oi); }
        }
        if (lane < cnt) { out[base + lane] = res; }
    }
    if (lane == 0) { *state = make_float2(offr, offi); }
}

// =====================================================================================================================
// AF chain: Deemphasis<stereo_t> (filter/deephasis.h:58-77): y[i] = alpha * x[i] + (1 - alpha) * y[i-1] per channel, state carried
// across pushes.  A first-order linear recurrence: one workgroup per VFO walks the push in super chunks of 256 * 8 frames; every
// work-item runs the recursion over its 8 frames from a zero carry, the chunk-end values are combined with a workgroup scan of
// the affine maps (m, a): y_end = m * y_in + a, and each work-item then re-runs the reference's exact expression from its true
// carry-in.  Only the carry-in differs in rounding from the sequential loop (~1e-7 relative; the filter is contractive).
// =====================================================================================================================
struct DeempJob {
    const float2* in;
    float2* out;
    int n;
    float alpha;      // KIND 0: de-emphasis alpha; KIND 1: DC-blocker rate
    const float2* state_in;  // KIND 0: lastOut (deephasis.h:72-73); KIND 1: offset (dc_blocker.h:57) as the block before left it, device resident
    float2* state_out;       // ... as this block leaves it (the host alternates two slots block by block: in pipelined mode pass 1 of block n + 1
                             // runs one launch behind pass 1 of block n and must neither wait for a third launch nor overwrite what is being read)
    float4* seg;      // [nseg] scratch: per segment (m, a.l, a.r, -): state_end = m * state_in + a (two buffers, alternating like the state)
    int nseg;         // segments of SDRPP_DEEMP_SEG frames
    int conj;         // KIND 1: negate the imaginary part of the output (dsp/math/conjugate.h) after the DC blocker
};
#define SDRPP_DEEMP_C 16
#define SDRPP_DEEMP_SEG (256 * SDRPP_DEEMP_C)

// Workgroup-wide composition of the per-work-item affine maps (Hillis-Steele): on return sm_m/sm_a[t] hold the map of work-items
// 0..t applied in order: (m2, a2) o (m1, a1) = (m2*m1, a2 + m2*a1).
__device__ __forceinline__ void deemph_block_scan(float* sm_m, float2* sm_a, int t, float m, float2 e) {
    sm_m[t] = m;
    sm_a[t] = e;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {
        float pm = 1.0f;
        float2 pa = make_float2(0.0f, 0.0f);
        const bool has = t >= d;
        if (has) {
            pm = sm_m[t - d];
            pa = sm_a[t - d];
        }
        __syncthreads();
        if (has) {
            const float mm = sm_m[t];
            const float2 aa = sm_a[t];
            sm_m[t] = mm * pm;
            sm_a[t] = make_float2(aa.x + mm * pa.x, aa.y + mm * pa.y);
        }
        __syncthreads();
    }
}

// First-order recurrences over a two-channel stream as a two-level scan.
//   KIND 0  Deemphasis<stereo_t>:   y[i] = alpha * x[i] + (1 - alpha) * y[i-1]                       (state = y)
//   KIND 1  DCBlocker<complex_t>:   out[i] = x[i] - off;  off += out[i] * rate   [then optional conj]  (state = off)
// Both states evolve by an affine map per sample (slope 1 - alpha / 1 - rate).
// PASS 0: segment maps from a zero state (grid: x = segment, y = job).  PASS 1: every segment composes the maps of the segments
// before it onto the carried state (a few dozen multiply-adds), then each work-item re-runs the reference's exact expression from
// its true carry-in; vfo_deemph_state_kernel stores the new state.
template <int KIND, int PASS>
__device__ __forceinline__ void vfo_deemph_body(const KIdx bid, float* smem, const DeempJob* __restrict__ jobs) {
    float* sm_m = smem;                                        // [256]
    float2* sm_a = reinterpret_cast<float2*>(smem + 256);      // [256]
    const DeempJob& job = jobs[bid.y];
    const int sg = bid.x;
    if (sg >= job.nseg) { return; }  // (the whole workgroup)
    constexpr int C = SDRPP_DEEMP_C;
    const int t = threadIdx.x;
    const float alpha = job.alpha, beta = 1.0f - alpha;
    const int i0 = sg * SDRPP_DEEMP_SEG + t * C;
    float2 x[C];
    float2 e = make_float2(0.0f, 0.0f);
    float m = 1.0f;
#pragma unroll
    for (int j = 0; j < C; j++) {
        const bool ok = i0 + j < job.n;
        x[j] = ok ? job.in[i0 + j] : make_float2(0.0f, 0.0f);
        if (ok) {
            if constexpr (KIND == 0) {
                e.x = (alpha * x[j].x) + (beta * e.x);
                e.y = (alpha * x[j].y) + (beta * e.y);
            }
            else {
                e.x += (x[j].x - e.x) * alpha;
                e.y += (x[j].y - e.y) * alpha;
            }
            m *= beta;
        }
    }
    deemph_block_scan(sm_m, sm_a, t, m, e);
    if constexpr (PASS == 0) {
        if (t == 255) { job.seg[sg] = make_float4(sm_m[255], sm_a[255].x, sm_a[255].y, 0.0f); }
    }
    else {
        float2 c0 = *job.state_in;  // carry into the push, then through the earlier segments (uniform: every work-item does the same)
        for (int q = 0; q < sg; q++) {
            const float4 g = job.seg[q];
            c0 = make_float2(g.y + g.x * c0.x, g.z + g.x * c0.y);
        }
        float2 y = c0;
        if (t > 0) { y = make_float2(sm_a[t - 1].x + sm_m[t - 1] * c0.x, sm_a[t - 1].y + sm_m[t - 1] * c0.y); }
#pragma unroll
        for (int j = 0; j < C; j++) {
            if (i0 + j < job.n) {
                if constexpr (KIND == 0) {
                    y.x = (alpha * x[j].x) + (beta * y.x);  // deephasis.h:66-69, same expression
                    y.y = (alpha * x[j].y) + (beta * y.y);
                    job.out[i0 + j] = y;
                }
                else {
                    const float2 o = make_float2(x[j].x - y.x, x[j].y - y.y);  // dc_blocker.h:56-57
                    y.x += o.x * alpha;
                    y.y += o.y * alpha;
                    job.out[i0 + j] = make_float2(o.x, job.conj ? -o.y : o.y);
                }
            }
        }
        // the state the NEXT block starts from: lastOut = out[n - 1] (deephasis.h:72-73) resp. the offset after the last sample — the work-item
        // that holds the last sample of the push has it in `y`
        if (sg == job.nseg - 1 && i0 < job.n && i0 + C >= job.n) { *job.state_out = y; }
    }
}
template <int KIND, int PASS>
__global__ __launch_bounds__(256) void vfo_deemph_kernel(const DeempJob* __restrict__ jobs) {
    __shared__ float sm[3 * 256];
    vfo_deemph_body<KIND, PASS>(kidx(blockIdx), sm, jobs);
}
// Conjugate alone (dsp/math/conjugate.h:12-15)
__global__ __launch_bounds__(256) void iq_conjugate_kernel(const float2* __restrict__ in, float2* __restrict__ out, int n) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const float2 x = in[i];
        out[i] = make_float2(x.x, -x.y);
    }
}

}  // namespace sdrpp_k
