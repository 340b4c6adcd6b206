// FIR filters on the vector units: the FM discriminator's phase, the direct form, the register-blocked form.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <sdrpp_gfx950.h>
#include <type_traits>
#include "fft_kernels.h"
#include "vfo_math.h"
#include "vfo_stream.h"

namespace sdrpp_k {

// =====================================================================================================================
// FM discriminator (quadrature.h:39-46): out[i] = normalizePhase(atan2f(x[i]) - atan2f(x[i-1])) * invDeviation — fused into the loads
// of the audio low-pass kernels (QUAD); this is its phase wrap.
// =====================================================================================================================
// atan2f for the discriminator: |error| <= 3e-7 rad against double precision (tests/host_cpp/test_device_math.cpp; libm's is ~1 ulp = 2.4e-7 at pi) in ~23 vector instructions instead of the
// ~53 of the library routine — the phase of every IF sample is taken on the way into the audio low-pass, which made this the
// largest single cost of that kernel.  Octant reduction to z = min/max in [0, 1], odd polynomial z * P(z^2) of degree 17
// (least-squares fit on Chebyshev nodes, weighted by z; max error 8.9e-8 in float arithmetic), then the usual reflections.
__device__ __forceinline__ float fm_phase(float y, float x) {
    const float ax = fabsf(x), ay = fabsf(y);
    const float mx = fmaxf(fmaxf(ax, ay), 1.17549435e-38f), mn = fminf(ax, ay);  // (0, 0) -> z = 0 -> phase 0 like atan2f
    const float z = mn * fast_rcp(mx);
    const float w = z * z;
    float p = 0.0023981390986591578f;
    p = fmaf(p, w, -0.014152348041534424f);
    p = fmaf(p, w, 0.03934541344642639f);
    p = fmaf(p, w, -0.07194384187459946f);
    p = fmaf(p, w, 0.10477539151906967f);
    p = fmaf(p, w, -0.1415480673313141f);
    p = fmaf(p, w, 0.19984884560108185f);
    p = fmaf(p, w, -0.33332523703575134f);
    p = fmaf(p, w, 0.9999998807907104f);
    float r = z * p;
    r = (ay > ax) ? 1.57079632679489662f - r : r;
    r = (x < 0.0f) ? 3.14159265358979324f - r : r;
    return copysignf(r, y);
}
__device__ __forceinline__ float normalize_phase(float d) {
    const float FL_PI = 3.1415926535f;  // math/constants.h:4, math/normalize_phase.h:6-9
    if (d > FL_PI) { d -= 2.0f * FL_PI; }
    else if (d <= -FL_PI) { d += 2.0f * FL_PI; }
    return d;
}

// =====================================================================================================================
// Register-blocked kernels (round-1 optimisation of the measured bottleneck).
//
// The generic FIR above issues one ds_read per two FMAs and is LDS-bound at ~10 TFLOP/s.  Here every work-item computes
// R = 8 consecutive outputs with a circular window of R registers: each input sample is read from LDS once and used for
// R outputs (R*R FMAs per R reads), taps are wave-uniform and arrive through scalar loads, R at a time.
//
// Decimation by D is handled as D ordinary FIRs over the polyphase components c_p[i] = x[base + D*i + p] with taps
// h_p[q] = h[D*q + p] (host lays them out phase-major, zero-padded to a multiple of R):
//      out[j] = sum_p sum_q h_p[q] * c_p[j + q]
// LDS image: component p, element e (tile-relative) at [p][e mod R][e div R]; work-item t reads elements t*R + m, i.e.
// [p][m mod R][t + m div R] — consecutive lanes, consecutive addresses.
// =====================================================================================================================
#define SDRPP_FIR_R 8
struct FirBJob {
    StreamIn in;
    float* out;
    const float* taps;  // [D][kp_pad], phase-major, zero padded
    int ntaps, log2_decim, off0, nout, kp_pad;
    float inv_deviation;  // QUAD only
};

// Decimating FIR on a complex stream whose window fits neither the matrix-core table nor an LDS tile (decimation 32 / 64 with hundreds
// of taps as a PLAIN filter: only in reference-rotator mode, where the first stage cannot be fused with the translation).  One output
// per work-item straight from global memory, k-ordered fmaf chain.  Correctness path of a parity mode, not tuned.
// REFORDER: the reference's own arithmetic — VOLK's generic dot product as DecimatingFIR::process calls it (decimating_fir.h:51-61):
// taps in order, product rounded, then added (two roundings per tap, no fused multiply-add).  The parity mode of the front end's
// pre-processing decimator (sdrpp_preproc_set_reference_order): bit-identical to the compiled reference.
template <bool REFORDER>
__device__ __forceinline__ void vfo_fir_direct_body(const KIdx bid, const KIdx gdim, const FirBJob* __restrict__ jobs) {
    const FirBJob& job = jobs[bid.y];
    const int D = 1 << job.log2_decim, kp = job.kp_pad;
    for (int j = bid.x * 256 + (int)threadIdx.x; j < job.nout; j += gdim.x * 256) {
        const int i0 = job.off0 + (j << job.log2_decim) - (job.ntaps - 1);
        float2 acc = make_float2(0.0f, 0.0f);
        for (int k = 0; k < job.ntaps; k++) {
            const float h = job.taps[(size_t)(k & (D - 1)) * kp + (size_t)(k >> job.log2_decim)];
            const float2 x = stream_load2(job.in, i0 + k);
            if constexpr (REFORDER) {
                const float pr = x.x * h, pi = x.y * h;  // (the translation unit is compiled with -ffp-contract=off: these stay products)
                acc.x = acc.x + pr;
                acc.y = acc.y + pi;
            }
            else { cmac(h, x, acc); }
        }
        reinterpret_cast<float2*>(job.out)[j] = acc;
    }
}
template <bool REFORDER>
__global__ __launch_bounds__(256) void vfo_fir_direct_kernel(const FirBJob* __restrict__ jobs) { vfo_fir_direct_body<REFORDER>(kidx(blockIdx), kidx(gridDim), jobs); }

// QUAD (WIDTH 1, decimation 1): the input stream is the complex IF and the FM discriminator (quadrature.h:39-46) runs while the
// tile is loaded — d[i] = normalizePhase(atan2f(x[i]) - atan2f(x[i-1])) * invDeviation — so the demodulated stream never goes
// to memory.  The reference keeps the previous phase as state; here it is recomputed from the IF history (atan2f(0, 0) = 0
// reproduces the reset state).
template <int WIDTH, bool STEREO, bool QUAD = false>
__device__ __forceinline__ void vfo_firb_body(const KIdx bid, float* smem, const int nthreads, const FirBJob* __restrict__ jobs) {  // nthreads: work-items of the workgroup that take part (a multiple of 64)
    constexpr int R = SDRPP_FIR_R;
    const FirBJob& job = jobs[bid.y];
    const int nall = (int)blockDim.x;  // every work-item of the workgroup loads, `nthreads` of them compute
    const int tile = nthreads * R;
    const int j0 = bid.x * tile;
    if (j0 >= job.nout) { return; }
    const int K = job.ntaps, lgD = job.log2_decim, D = 1 << lgD, kp = job.kp_pad;
    const int P1 = nthreads + kp / R + 1;  // columns per (phase, residue) row
    const int P2 = R * P1;
    // component elements needed per phase: tile + kp - 1 (+R-1 preload slack) -> all inside R * P1
    const int ncomp = R * P1;
    const int base = job.off0 + j0 * D - (K - 1);  // stream index of component 0, element 0
    const int nvalid = (tile - 1) * D + K;         // samples a full tile really needs; the rest is zero-filled
    typedef typename std::conditional<WIDTH == 2, float2, float>::type T;
    T* xs = reinterpret_cast<T*>(smem);
    if constexpr (QUAD) {
        float* phase = smem + ncomp;  // phase[i] = atan2f(x[base - 1 + i]), i = 0 .. nvalid
        constexpr int UQ = 4;
        for (int s0 = threadIdx.x; s0 <= nvalid; s0 += nall * UQ) {
            float2 x[UQ];
#pragma unroll
            for (int u = 0; u < UQ; u++) { x[u] = stream_load2_nb(job.in, base - 1 + s0 + u * nall, s0 + u * nall <= nvalid); }
#pragma unroll
            for (int u = 0; u < UQ; u++) {
                if (s0 + u * nall <= nvalid) { phase[s0 + u * nall] = fm_phase(x[u].y, x[u].x); }
            }
        }
        __syncthreads();
        for (int s = threadIdx.x; s < ncomp; s += nall) {
            const float v = (s < nvalid) ? normalize_phase(phase[s + 1] - phase[s]) * job.inv_deviation : 0.0f;
            xs[(s & (R - 1)) * P1 + (s >> 3)] = v;
        }
    }
    else {
        // Eight loads in flight per work-item before the first LDS store, none behind a branch (stream_load*_nb): a tile of a decimator by 8 is
        // ~17 samples per work-item, and one guarded load per loop iteration made that 17 memory round trips one after the other — the whole
        // 18 us life of this role's workgroups in cfg 4's tick, 512 of them (round 5; same values, same order of everything that is rounded).
        constexpr int U = 8;
        for (int s0 = threadIdx.x; s0 < ncomp * D; s0 += nall * U) {
            T v[U];
#pragma unroll
            for (int u = 0; u < U; u++) {
                const int s = s0 + u * nall;
                if constexpr (WIDTH == 2) { v[u] = stream_load2_nb(job.in, base + s, s < nvalid); }
                else { v[u] = stream_load1_nb(job.in, base + s, s < nvalid); }
            }
#pragma unroll
            for (int u = 0; u < U; u++) {
                const int s = s0 + u * nall;
                if (s < ncomp * D) {
                    const int p = s & (D - 1), e = s >> lgD;
                    xs[p * P2 + (e & (R - 1)) * P1 + (e >> 3)] = v[u];
                }
            }
        }
    }
    __syncthreads();
    const int t = threadIdx.x;
    if (t >= nthreads) { return; }  // (a role of the tick kernel: the workgroup is wider than the tile; everybody helped to load it and met the barriers)
    const UniformF32 taps = as_uniform(job.taps);
    T acc[R];
#pragma unroll
    for (int r = 0; r < R; r++) {
        if constexpr (WIDTH == 2) { acc[r] = make_float2(0.0f, 0.0f); }
        else { acc[r] = 0.0f; }
    }
    for (int p = 0; p < D; p++) {
        const T* xp = xs + p * P2 + t;
        T w[R];
#pragma unroll
        for (int m = 0; m < R - 1; m++) { w[m] = xp[m * P1]; }  // elements 0 .. R-2 (m div R == 0)
        for (int q0 = 0; q0 < kp; q0 += R) {
            const int col = (q0 >> 3);
#pragma unroll
            for (int u = 0; u < R; u++) {
                // element m = q0 + u + R - 1 -> residue (u - 1) mod R, column col + (u >= 1)
                const int res = (u + R - 1) & (R - 1);
                w[res] = xp[res * P1 + col + (u >= 1 ? 1 : 0)];
                const float h = taps[p * kp + q0 + u];
#pragma unroll
                for (int r = 0; r < R; r++) {
                    const T x = w[(u + r) & (R - 1)];
                    if constexpr (WIDTH == 2) { cmac(h, x, acc[r]); }
                    else { acc[r] = fmaf(h, x, acc[r]); }
                }
            }
        }
    }
    const int jo = j0 + t * R;
#pragma unroll
    for (int r = 0; r < R; r++) {
        if (jo + r < job.nout) {
            if constexpr (WIDTH == 2) { global_store_f32x2(reinterpret_cast<float2*>(job.out), jo + r, acc[r]); }  // (explicit GLOBAL stores: FLAT ones as a tick role)
            else if constexpr (STEREO) { global_store_f32x2(reinterpret_cast<float2*>(job.out), jo + r, make_float2(acc[r], acc[r])); }
            else { global_store_f32_boff(job.out, (unsigned)(jo + r) * 4u, acc[r]); }
        }
    }
}
template <int WIDTH, bool STEREO, bool QUAD = false>
__global__ __launch_bounds__(256) void vfo_firb_kernel(const FirBJob* __restrict__ jobs) {
    HIP_DYNAMIC_SHARED(float, smem)
    vfo_firb_body<WIDTH, STEREO, QUAD>(kidx(blockIdx), smem, (int)blockDim.x, jobs);
}

}  // namespace sdrpp_k
