// The first stage of a VFO: frequency translation folded into the first decimating FIR (LDS-tiled and direct forms), rotation alone.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <sdrpp_gfx950.h>
#include "fft_kernels.h"
#include "vfo_math.h"

namespace sdrpp_k {

// =====================================================================================================================
// Stage 1: frequency translation folded into the first decimating FIR, VT VFOs per work-item sharing one LDS input tile
// =====================================================================================================================
// Reference:  r[n] = x[n] * e^{j(phi0 + n*theta)}  (rotator), then  y[j] = sum_k h[k] * r[i0 + k],  i0 = off0 + j*D - (K-1).
// Same sum:   y[j] = e^{j(phi0 + (i0 + kc)*theta)} * sum_k g[k] * x[i0 + k],   g[k] = h[k] * e^{j(k - kc)*theta}
// with complex taps g (host, double precision -> float) and ONE phasor per output instead of one per input sample.
// theta = arg(phaseDelta) of the reference's float phaseDelta, phi0 accumulated on the host in double.
#define SDRPP_S1_MAX_VT 8
struct Stage1Job {
    int nv;                  // VFOs handled by this job (<= VT of the launch)
    int ntaps, log2_decim, off0, nout;
    int min_idx;             // samples before this push-relative index read as zero (a VFO added or reset mid-stream starts
                             // from an all-zero history: fir.h:24-26 clears the delay line)
    int anchor;              // the index phi0 belongs to (0 = the block's first sample; a push of a launch group: where ITS samples start)
    const float2* ctaps;     // [(ntaps+1)/2][VT] modulated tap pairs (see stage1_accumulate), VFO index fastest
    double theta[SDRPP_S1_MAX_VT];  // turns per input sample
    double phi0[SDRPP_S1_MAX_VT];   // turns at push-relative sample index 0
    float2* out[SDRPP_S1_MAX_VT];
};


// Symmetric-tap form of the translated FIR.  Every stage of the reference's decimation plans is linear phase (h[k] == h[K-1-k],
// checked on the host; asymmetric taps fall back to nothing here — the host refuses them), so with the modulation centred on
// the filter, g[K-1-k] = conj(g[k]) and
//     g[k]*a + conj(g[k])*b = g.re * (a + b) + j * g.im * (a - b)            (a = x[i0+k], b = x[i0+K-1-k])
// i.e. FOUR FMAs per tap PAIR and VFO instead of eight; the sum/difference are shared by all VT VFOs of the work-item.
// ctaps: [npairs][VT] float2 (g.re, g.im), npairs = (K+1)/2; an odd K has its centre tap as a last "pair" with b = 0, g.im = 0.
template <int VT>
__device__ __forceinline__ void stage1_accumulate(const float2* xs, int pitch, int lgD, int K, int j, const UniformF32 g, float2 (&acc)[VT]) {
    const int D = 1 << lgD;
    const int npairs = (K + 1) >> 1;
    const bool odd = (K & 1) != 0;
    for (int k = 0; k < npairs; k++) {
        const int kb = K - 1 - k;
        const float2 a = xs[(k & (D - 1)) * pitch + (k >> lgD) + j];
        float2 b = xs[(kb & (D - 1)) * pitch + (kb >> lgD) + j];
        if (odd && k == npairs - 1) { b = make_float2(0.0f, 0.0f); }
        const float sr = a.x + b.x, si = a.y + b.y, dr = a.x - b.x, di = a.y - b.y;
#pragma unroll
        for (int v = 0; v < VT; v++) {
            const float gr = g[2 * (k * VT + v)], gi = g[2 * (k * VT + v) + 1];
            acc[v].x = fmaf(gr, sr, acc[v].x);
            acc[v].x = fmaf(-gi, di, acc[v].x);
            acc[v].y = fmaf(gr, si, acc[v].y);
            acc[v].y = fmaf(gi, dr, acc[v].y);
        }
    }
}


// Compile-time (K, log2 D) variant: fully unrolled, so every LDS offset is an instruction immediate and the tap fetches are
// s_load_dwordx16 with constant offsets that the scheduler can hoist ahead of their use — no scalar address arithmetic at all
// (the generic loop spends as many SALU as VALU instructions; one scalar unit serves the four SIMDs of a CU).
template <int VT, int K, int LGD>
__device__ __forceinline__ void stage1_accumulate_static(const float2* xs, int pitch, int j, const UniformF32 g, float2 (&acc)[VT]) {
    constexpr int D = 1 << LGD;
    constexpr int NP = (K + 1) / 2;
    const float2* xj = xs + j;
#pragma unroll
    for (int k = 0; k < NP; k++) {
        const int kb = K - 1 - k;
        const float2 a = xj[(k & (D - 1)) * pitch + (k >> LGD)];
        float2 b = xj[(kb & (D - 1)) * pitch + (kb >> LGD)];
        if ((K & 1) && k == NP - 1) { b = make_float2(0.0f, 0.0f); }
        const float sr = a.x + b.x, si = a.y + b.y, dr = a.x - b.x, di = a.y - b.y;
#pragma unroll
        for (int v = 0; v < VT; v++) {
            const float gr = g[2 * (k * VT + v)], gi = g[2 * (k * VT + v) + 1];
            acc[v].x = fmaf(gr, sr, acc[v].x);
            acc[v].x = fmaf(-gi, di, acc[v].x);
            acc[v].y = fmaf(gr, si, acc[v].y);
            acc[v].y = fmaf(gi, dr, acc[v].y);
        }
    }
}

// grid = (ceil(max nout / TILE), njobs); block = TILE work-items; dynamic LDS = D * pitch float2 with
// pitch = TILE + ceil((K-1)/D) + 1.  LDS image is de-interleaved by decimation phase: sample s of the tile lives at
// [s mod D][s div D], so lane j reads x[j*D + k] at [k mod D][j + k div D] — consecutive lanes, consecutive addresses.
// (also a role of the tick kernel — TR_S1_1, round 5: banks too small for the matrix front end stay pipelined; `tile` work-items compute, all `nall` of the
// workgroup load)
template <int VT>
__device__ __forceinline__ void vfo_stage1_body(const KIdx bid, float2* xs, const int tile, const int nall, const IqSrc& src, const Stage1Job* __restrict__ jobs) {
    const Stage1Job& job = jobs[bid.y];
    const int j0 = bid.x * tile;
    if (j0 >= job.nout) { return; }
    const int K = job.ntaps, lgD = job.log2_decim, D = 1 << lgD;
    const int extra = (K - 1 + D - 1) >> lgD;
    const int pitch = tile + extra + 1;
    const int nsamp = (tile - 1) * D + K;
    const long long base = (long long)job.off0 + (long long)j0 * D - (K - 1);  // push-relative index of tile sample 0
    for (int s = threadIdx.x; s < nsamp; s += nall) {
        const long long gi = base + s;
        xs[(s & (D - 1)) * pitch + (s >> lgD)] = (gi < job.min_idx) ? make_float2(0.0f, 0.0f) : iq_load_clamped(src, gi);
    }
    __syncthreads();
    const int j = threadIdx.x;
    if (j >= tile) { return; }
    float2 acc[VT];
#pragma unroll
    for (int v = 0; v < VT; v++) { acc[v] = make_float2(0.0f, 0.0f); }
    stage1_accumulate<VT>(xs, pitch, lgD, K, j, as_uniform(job.ctaps), acc);  // taps are wave-uniform: scalar loads
    if (j0 + j >= job.nout) { return; }
    const double centre = (double)(base + (long long)j * D - job.anchor) + 0.5 * (double)(K - 1);
#pragma unroll
    for (int v = 0; v < VT; v++) {
        if (v < job.nv) {
            float sn, cs;
            turn_sincos(fma(centre, job.theta[v], job.phi0[v]), sn, cs);
            float2 y;
            y.x = fmaf(acc[v].x, cs, -(acc[v].y * sn));
            y.y = fmaf(acc[v].x, sn, acc[v].y * cs);
            job.out[v][j0 + j] = y;
        }
    }
}
template <int VT>
__global__ __launch_bounds__(256) void vfo_stage1_kernel(IqSrc src, const Stage1Job* __restrict__ jobs) {
    HIP_DYNAMIC_SHARED(float2, xs)
    vfo_stage1_body<VT>(kidx(blockIdx), xs, (int)blockDim.x, (int)blockDim.x, src, jobs);
}

// Large first-stage decimation (D >= 32: the 61.44 MS/s plans decimate by 64 with 257..400 taps).  An LDS tile for even 64
// outputs would be ~36 KiB, leaving one wavefront per SIMD.  Consecutive outputs start D samples apart, so there is almost
// no overlap between neighbouring lanes to exploit anyway: every lane streams its own K contiguous samples straight from
// global memory (each 64-byte line is consumed over 8 iterations and stays in L1), no LDS, full occupancy.  Reuse is across
// the VT VFOs of the work-item, exactly as in the tiled kernel.
template <int VT>
__device__ __forceinline__ void vfo_stage1_direct_body(const KIdx bid, const IqSrc& src, const Stage1Job* __restrict__ jobs) {  // (256 work-items; role TR_S1D_1)
    const Stage1Job& job = jobs[bid.y];
    const int j = bid.x * 256 + (int)threadIdx.x;
    const int K = job.ntaps, lgD = job.log2_decim;
    const int jc = (j < job.nout) ? j : (job.nout - 1);  // lanes past the end redo the last output (no divergence), never store
    if (job.nout <= 0) { return; }
    const long long i0 = (long long)job.off0 + ((long long)jc << lgD) - (K - 1);
    const int npairs = (K + 1) >> 1;
    const bool odd = (K & 1) != 0;
    const UniformF32 g = as_uniform(job.ctaps);
    float2 acc[VT];
#pragma unroll
    for (int v = 0; v < VT; v++) { acc[v] = make_float2(0.0f, 0.0f); }
    // block-uniform fast path: every window of this block lies inside the current push
    const long long blk_first = (long long)job.off0 + ((long long)(bid.x * 256) << lgD) - (K - 1);
    const long long blk_last = (long long)job.off0 + ((long long)min(bid.x * 256 + 255, job.nout - 1) << lgD);
    const bool inside = blk_first >= 0 && blk_first >= job.min_idx && blk_last < src.n_cur;
    if (inside) {
        const float2* __restrict__ xa = src.cur + i0;
        for (int k = 0; k < npairs; k++) {
            const float2 a = xa[k];
            float2 b = xa[K - 1 - k];
            if (odd && k == npairs - 1) { b = make_float2(0.0f, 0.0f); }
            const float sr = a.x + b.x, si = a.y + b.y, dr = a.x - b.x, di = a.y - b.y;
#pragma unroll
            for (int v = 0; v < VT; v++) {
                const float gr = g[2 * (k * VT + v)], gi = g[2 * (k * VT + v) + 1];
                acc[v].x = fmaf(gr, sr, acc[v].x);
                acc[v].x = fmaf(-gi, di, acc[v].x);
                acc[v].y = fmaf(gr, si, acc[v].y);
                acc[v].y = fmaf(gi, dr, acc[v].y);
            }
        }
    }
    else {
        for (int k = 0; k < npairs; k++) {
            const long long ia = i0 + k, ib = i0 + K - 1 - k;
            const float2 a = (ia < job.min_idx) ? make_float2(0.0f, 0.0f) : iq_load_clamped(src, ia);
            float2 b = (ib < job.min_idx) ? make_float2(0.0f, 0.0f) : iq_load_clamped(src, ib);
            if (odd && k == npairs - 1) { b = make_float2(0.0f, 0.0f); }
            const float sr = a.x + b.x, si = a.y + b.y, dr = a.x - b.x, di = a.y - b.y;
#pragma unroll
            for (int v = 0; v < VT; v++) {
                const float gr = g[2 * (k * VT + v)], gi = g[2 * (k * VT + v) + 1];
                acc[v].x = fmaf(gr, sr, acc[v].x);
                acc[v].x = fmaf(-gi, di, acc[v].x);
                acc[v].y = fmaf(gr, si, acc[v].y);
                acc[v].y = fmaf(gi, dr, acc[v].y);
            }
        }
    }
    if (j >= job.nout) { return; }
    const double centre = (double)(i0 - job.anchor) + 0.5 * (double)(K - 1);
#pragma unroll
    for (int v = 0; v < VT; v++) {
        if (v < job.nv) {
            float sn, cs;
            turn_sincos(fma(centre, job.theta[v], job.phi0[v]), sn, cs);
            job.out[v][j] = make_float2(fmaf(acc[v].x, cs, -(acc[v].y * sn)), fmaf(acc[v].x, sn, acc[v].y * cs));
        }
    }
}
template <int VT>
__global__ __launch_bounds__(256) void vfo_stage1_direct_kernel(IqSrc src, const Stage1Job* __restrict__ jobs) { vfo_stage1_direct_body<VT>(kidx(blockIdx), src, jobs); }

// Rotation only (VFOs whose output rate is above half the input rate have no decimation stage: power_decimator.h:53-56).
struct RotJob {
    double theta, phi0;
    float2* out;
    int n;
};
__device__ __forceinline__ void vfo_rotate_body(const KIdx bid, const KIdx gdim, const IqSrc& src, const RotJob* __restrict__ jobs) {
    const RotJob& job = jobs[bid.y];
    for (int i = bid.x * blockDim.x + threadIdx.x; i < job.n; i += gdim.x * blockDim.x) {
        float sn, cs;
        turn_sincos(fma((double)i, job.theta, job.phi0), sn, cs);
        job.out[i] = cmul(iq_load(src, i), cs, sn);
    }
}
__global__ __launch_bounds__(256) void vfo_rotate_kernel(IqSrc src, const RotJob* __restrict__ jobs) { vfo_rotate_body(kidx(blockIdx), kidx(gridDim), src, jobs); }

}  // namespace sdrpp_k
