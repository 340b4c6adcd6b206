// Polyphase rational resampler with many phases, cycle-major.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <sdrpp_gfx950.h>
#include "fft_kernels.h"
#include "vfo_math.h"
#include "vfo_stream.h"
#include "vfo_resample_kernels.h"

namespace sdrpp_k {

// =====================================================================================================================
// Polyphase resampler with many phases (the AF chain's 96/125): cycle-major.  A tile = CT whole phase cycles (CT * L outputs,
// CT * M inputs); lane j owns cycle j, a wavefront walks over phases r = w, w + 4, ...: within a wavefront the phase — hence
// the tap row — is uniform (scalar loads) and all L phases reuse ONE LDS window of CT * M + tpp input samples.
// =====================================================================================================================
// `cap2g` = LDS window in float2 (low 24 bits) | phase groups G - 1 (bits 24 ..): a tile's L phases can be dealt out over G workgroups (each loads
// the tile's window and walks phases wv + 4 g, wv + 4 g + 4 G, ...) — what a wavefront does one after the other is L / 4 phases x tpp taps, the
// whole life of the workgroup, and at the reference's block size a block's AF output is 2-3 cycles: 3 busy lanes walking 24 phases x 99 taps.
__device__ __forceinline__ void vfo_polyc_body(const KIdx bid, float2* xsc, const PolyJob* __restrict__ jobs, int cap2g) {
    const PolyJob& job = jobs[bid.y];
    const int L = job.interp, M = job.decim, tpp = job.tpp;
    const int cap2 = cap2g & 0xffffff, G = (cap2g >> 24) + 1;
    int CT = (cap2 - tpp - M) / M;  // cycles per tile: window (CT - 1) * M + o_max + tpp <= cap2, o_max <= M
    if (CT > 64) { CT = 64; }
    const int g = bid.x % G;
    const int c0 = (bid.x / G) * CT;
    if ((long long)c0 * L >= job.nout) { return; }
    const int first = job.off0 + c0 * M - (tpp - 1);
    const int nwin = CT * M + M + tpp;
    for (int s = threadIdx.x; s < nwin; s += 256) { xsc[s] = stream_load2(job.in, first + s); }
    __syncthreads();
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int r = wv + 4 * g; r < L; r += 4 * G) {
        const int A = job.phase0 + r * M, ph = A % L, o = A / L;
        const UniformF32 taps = as_uniform(job.bank + (size_t)ph * tpp);
        const float2* xp = xsc + lane * M + o;
        float2 acc = make_float2(0.0f, 0.0f);
        if (lane < CT) {
            for (int k = 0; k < tpp; k++) {
                const float h = taps[k];
                cmac(h, xp[k], acc);
            }
            const long long n = (long long)(c0 + lane) * L + r;
            if (n < job.nout) { global_store_f32x2(job.out, n, acc); }
        }
    }
}
__global__ __launch_bounds__(256) void vfo_polyc_kernel(const PolyJob* __restrict__ jobs, int cap2) {
    HIP_DYNAMIC_SHARED(float2, xsc)
    vfo_polyc_body(kidx(blockIdx), xsc, jobs, cap2);
}

}  // namespace sdrpp_k
