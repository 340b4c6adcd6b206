// Polyphase rational resampler: one output per work-item, and register-blocked over one phase cycle.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <sdrpp_gfx950.h>
#include "fft_kernels.h"
#include "vfo_math.h"
#include "vfo_stream.h"

namespace sdrpp_k {

// =====================================================================================================================
// Polyphase rational resampler (polyphase_resampler.h:75-93):
//   A_n = phase0 + n*M;  out[n] = sum_k bank[A_n mod L][k] * in[offset0 + A_n div L + k - (tpp-1)]
// bank[(L-1) - (i mod L)][i div L] = taps[i] (polyphase_bank.h:31-34) is laid out [phase][tpp] on the host.
// =====================================================================================================================
struct PolyJob {
    StreamIn in;
    float2* out;
    const float* bank;  // [interp][tpp]
    int interp, decim, tpp, phase0, off0, nout;
};

__device__ __forceinline__ void vfo_poly_body(const KIdx bid, float2* xs, const PolyJob* __restrict__ jobs) {  // 256 work-items, one output each (role TR_POLY)
    const PolyJob& job = jobs[bid.y];
    constexpr int tile = 256;
    const int n0 = bid.x * tile;
    if (n0 >= job.nout) { return; }
    const int L = job.interp, M = job.decim, tpp = job.tpp;
    const long long a0 = (long long)job.phase0 + (long long)n0 * M;
    int nlast = n0 + tile - 1;
    if (nlast >= job.nout) { nlast = job.nout - 1; }
    const long long a1 = (long long)job.phase0 + (long long)nlast * M;
    const int first = job.off0 + (int)(a0 / L) - (tpp - 1);  // stream index of the first sample this tile needs
    const int nsamp = (int)(a1 / L) - (int)(a0 / L) + tpp;
    for (int s = threadIdx.x; s < nsamp; s += tile) { xs[s] = stream_load2(job.in, first + s); }
    __syncthreads();
    const int n = n0 + threadIdx.x;
    if (n >= job.nout) { return; }
    const long long a = (long long)job.phase0 + (long long)n * M;
    const int ph = (int)(a % L);
    const int rel = (int)(a / L) - (int)(a0 / L);
    const float* __restrict__ t = job.bank + (size_t)ph * tpp;
    float2 acc = make_float2(0.0f, 0.0f);
    for (int k = 0; k < tpp; k++) {
        const float2 x = xs[rel + k];
        cmac(t[k], x, acc);
    }
    job.out[n] = acc;
}
__global__ __launch_bounds__(256) void vfo_poly_kernel(const PolyJob* __restrict__ jobs) {
    HIP_DYNAMIC_SHARED(float2, xs)
    vfo_poly_body(kidx(blockIdx), xs, jobs);
}

// Polyphase resampler, register-blocked over one full phase cycle per work-item: outputs n = c*L + r (r = 0..L-1) of cycle c
// use phases (phase0 + r*M) mod L and input offsets c*M + o_r, o_r = (phase0 + r*M) div L — the SAME (phase, o_r) pattern for
// every cycle, so the taps are wave-uniform.  The host tabulates, for every phase0, cyc[m][r] = bank[phase_r][m - o_r] (0
// outside the filter), m = 0 .. tpp + M - 1; a work-item walks its tpp + M inputs once, doing LMAX FMAs (complex: 2x) per read.
struct PolyBJob {
    StreamIn in;
    float2* out;
    const float* cyc;  // [rows][LMAX] for this push's phase0
    int interp, decim, tpp, off0, nout, rows;
};

template <int LMAX, bool LINEAR>
__global__ __launch_bounds__(256) void vfo_polyb_kernel(const PolyBJob* __restrict__ jobs) {
    HIP_DYNAMIC_SHARED(float2, xs)
    const PolyBJob& job = jobs[blockIdx.y];
    const int nthreads = blockDim.x;
    const int L = job.interp, M = job.decim, rows = job.rows;
    const int c0 = blockIdx.x * nthreads;  // first cycle of this block
    if (c0 * L >= job.nout) { return; }
    const int P1 = nthreads + rows / M + 2;  // columns per residue row (de-interleaved layout)
    const int first = job.off0 + c0 * M - (job.tpp - 1);
    const int need = (nthreads - 1) * M + rows;
    if constexpr (LINEAR) {
        // odd M: lanes read t*M + m, a stride of 2*M dwords — conflict-free for ds_read_b64 (gcd(2M, 64) = 2), so the tile is
        // stored as is and the row loop needs no address arithmetic
        for (int s = threadIdx.x; s < need; s += nthreads) { xs[s] = stream_load2(job.in, first + s); }
    }
    else {
        for (int s = threadIdx.x; s < M * P1; s += nthreads) {
            const float2 v = (s < need) ? stream_load2(job.in, first + s) : make_float2(0.0f, 0.0f);
            xs[(s % M) * P1 + (s / M)] = v;  // element s of the tile lives at [s mod M][s div M]
        }
    }
    __syncthreads();
    const int t = threadIdx.x;
    const UniformF32 cyc = as_uniform(job.cyc);
    float2 acc[LMAX];
#pragma unroll
    for (int r = 0; r < LMAX; r++) { acc[r] = make_float2(0.0f, 0.0f); }
    if constexpr (LINEAR) {
        const float2* xp = xs + t * M;
#pragma unroll 4
        for (int m = 0; m < rows; m++) {
            const float2 x = xp[m];
#pragma unroll
            for (int r = 0; r < LMAX; r++) {
                cmac(cyc[m * LMAX + r], x, acc[r]);
            }
        }
    }
    else {
        int res = 0, col = t;  // element t*M + m -> residue m mod M, column t + m div M
        for (int m = 0; m < rows; m++) {
            const float2 x = xs[res * P1 + col];
#pragma unroll
            for (int r = 0; r < LMAX; r++) {
                cmac(cyc[m * LMAX + r], x, acc[r]);
            }
            if (++res == M) { res = 0; col++; }
        }
    }
    const int n0 = (c0 + t) * L;
#pragma unroll
    for (int r = 0; r < LMAX; r++) {
        if (r < L && n0 + r < job.nout) { job.out[n0 + r] = acc[r]; }
    }
}

}  // namespace sdrpp_k
