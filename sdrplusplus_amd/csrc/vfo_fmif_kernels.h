// FM IF noise reduction on the matrix cores: a kind of the wavefront-job role (vfo_ifchain_kernels.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <sdrpp_gfx950.h>
#include "vfo_stream.h"

namespace sdrpp_k {

// =====================================================================================================================
// FMIF (noise_reduction/fm_if.h:45-77), the last block of the radio's IF chain.  For every IF sample i, with N = bins:
//     X_i[k] = sum_n w[n] * x[i - (N-1) + n] * e^{-j 2 pi k n / N}        (window, forward DFT over the last N samples)
//     idx    = first k of maximal sqrtf(re^2 + im^2)                      (volk's index_max: strict >)
//     out[i] = X_i[idx] * e^{+j 2 pi idx floor(N/2) / N}                  (the un-normalised backward DFT of that one bin, read at N/2)
// No state but the delay line, so the block is parallel over samples.  The output twiddle is folded into the matrix,
//     Y[k, i] = sum_n A[k, n] * x[i - (N-1) + n],      A[k, n] = w[n] * e^{-j 2 pi k (n - floor(N/2)) / N}      (|Y| = |X|: the argmax runs on Y, the output IS Y[idx])
// and the transform of 32 consecutive samples is one dense 32 x 32 complex matrix (designed in double on the host, sdrpp_host::fmifMatrix,
// zero rows and columns above N) applied to the Hankel view of the stream: four real 32 x 32 x 2 products per pair of window offsets,
//     Yr += Ar * xr + Ai * (-xi)        Yi += Ai * xr + Ar * xi
// with A in registers for the whole job (lane l holds A[k = l & 31][n = 2 t + (l >> 5)], t < 16) and the B operand W[j + 2 t + (l >> 5)] read
// from the wavefront's LDS window as (re, im) pairs: consecutive lanes read consecutive 8-byte words, no bank conflict.  Only the
// ceil(N / 2) steps that hold a non-zero column are issued.  A column's 32 bins lie in 16 accumulator registers of lane j and 16 of lane
// j + 32: the argmax runs within the lane first (ascending k, strict >), then across the two halves through LDS (equal magnitudes: the lower
// k), so exact ties resolve as in the reference; a zero row never beats a non-zero maximum, and an all-zero window gives bin 0 and 0.
// Every output is the n-ascending fmaf chain of its own column — the same value wherever the segment or the block was cut.
// One WAVEFRONT per segment of SDRPP_FMIF_SEG samples (a wave job each, all of a block reading the VFO's one record).
// =====================================================================================================================
#define SDRPP_FMIF_TILE 32
#define SDRPP_FMIF_SEG 256
#ifndef SDRPP_WAVE_LDS_FLOATS
#error "a part of vfo_ifchain_kernels.h, the role's header: include that one"
#endif
#define SDRPP_FMIF_LDS_FLOATS ((SDRPP_FMIF_SEG + SDRPP_FMIF_TILE) * 2 + 64 * 4)  // of the wavefront's share of the role's LDS: the window, then the exchange of the argmax

// One record per VFO and block (WK_FMIF); a wave job is one segment of it, its first sample in WaveJob::arg.
struct FmifJob {
    const float2* in;   // the input stream's data of this push (RxVFO::out, or the blanker / squelch job's output)
    float2* out;        // the chain's own output
    int n;
    int bins;
    const float* hist;  // the input stream's history (StreamIn)
    int hist_len;
    const float* tab;   // [2][32][32]: re / im of A[k][n] at [n][k]
};

__device__ __forceinline__ void vfo_fmif_body(const FmifJob& job, int lo, float* smem) {
    const int lane = threadIdx.x & 63, wv = (int)threadIdx.x >> 6;
    const int j = lane & 31, h = lane >> 5;
    float2* W = reinterpret_cast<float2*>(smem + wv * SDRPP_WAVE_LDS_FLOATS);
    float4* EX = reinterpret_cast<float4*>(smem + wv * SDRPP_WAVE_LDS_FLOATS + (SDRPP_FMIF_SEG + SDRPP_FMIF_TILE) * 2);
    const int N = job.bins;
    const int cnt = min(job.n - lo, SDRPP_FMIF_SEG);  // samples of this segment
    const int nst = (N + 1) >> 1;                     // matrix steps that hold a non-zero column
    const StreamIn in{ reinterpret_cast<const float*>(job.in), job.hist, job.hist_len, job.n };
    // W[p] = x[lo - (N-1) + p] for p < cnt + N - 1; zero behind it (an odd N pairs its last column with a zero one: what it multiplies must be finite)
    float2 pf[(SDRPP_FMIF_SEG + SDRPP_FMIF_TILE) / 64 + 1];
#pragma unroll
    for (int q = 0; q < (SDRPP_FMIF_SEG + SDRPP_FMIF_TILE) / 64 + 1; q++) {
        const int p = q * 64 + lane, i = lo - (N - 1) + p;
        pf[q] = stream_load2_nb(in, i, p < cnt + N - 1 && i >= -in.hist_len);
    }
    float ar[16], ai[16];
#pragma unroll
    for (int t = 0; t < 16; t++) {
        ar[t] = global_load_f32(job.tab, (2 * t + h) * 32 + j);
        ai[t] = global_load_f32(job.tab, 1024 + (2 * t + h) * 32 + j);
    }
#pragma unroll
    for (int q = 0; q < (SDRPP_FMIF_SEG + SDRPP_FMIF_TILE) / 64 + 1; q++) {
        const int p = q * 64 + lane;
        if (p < SDRPP_FMIF_SEG + SDRPP_FMIF_TILE) { W[p] = pf[q]; }
    }
    wave_sync();
    for (int t0 = 0; t0 < cnt; t0 += SDRPP_FMIF_TILE) {
        f32x16 yr = mfma_zero(), yi = mfma_zero();
        const float2* B = W + t0 + j + h;
#pragma unroll
        for (int t = 0; t < 16; t++) {
            if (t < nst) {  // (wave-uniform)
                const float2 x = B[2 * t];
                yr = mfma_32x32x2(ar[t], x.x, yr);
                yi = mfma_32x32x2(ai[t], x.x, yi);
                yr = mfma_32x32x2(ai[t], -x.y, yr);
                yi = mfma_32x32x2(ar[t], x.y, yi);
            }
        }
        // register r of this lane: bin k = (r & 3) + 8 * (r >> 2) + 4 * h of sample t0 + j
        float best = -1.0f, bre = 0.0f, bim = 0.0f;
        int bk = 0;
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const float m = sqrtf((yr[r] * yr[r]) + (yi[r] * yi[r]));
            if (m > best) {
                best = m;
                bk = (r & 3) + 8 * (r >> 2) + 4 * h;
                bre = yr[r];
                bim = yi[r];
            }
        }
        EX[lane] = make_float4(best, __int_as_float(bk), bre, bim);
        wave_sync();
        const float4 o = EX[lane ^ 32];
        const int ok = __float_as_int(o.y);
        if (o.x > best || (o.x == best && ok < bk)) {
            bre = o.z;
            bim = o.w;
        }
        if (h == 0 && t0 + j < cnt) { global_store_f32x2(job.out, lo + t0 + j, make_float2(bre, bim)); }
        wave_sync();  // (the next tile overwrites the exchange)
    }
}

}  // namespace sdrpp_k
