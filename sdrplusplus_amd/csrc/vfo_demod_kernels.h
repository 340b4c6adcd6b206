// AM / SSB demodulators: the parallel part, the AGC, the sequential tails.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <sdrpp_gfx950.h>
#include "fft_kernels.h"
#include "vfo_math.h"

namespace sdrpp_k {

// =====================================================================================================================
// Sequential tails at IF rate — one work-item per VFO, exactly the reference's per-sample recursions:
//   AM  (am.h:101-131): [carrier AGC] -> |x| -> DC blocker (dc_blocker.h:54-60) -> [audio AGC] -> (LPF runs afterwards as a FIR job)
//   SSB (ssb.h:77-92) : second translation (closed-form NCO) -> Re{} -> AGC (agc.h:70-109) -> {v, v}
// The AGC look-ahead on clipping scans to the end of the reference block (SeqJob::bounds; without them: to the end of the push).
// =====================================================================================================================
struct AgcState {
    float set_point, attack, inv_attack, decay, inv_decay, max_gain, max_output_amp, amp;
};
// Parallel part of AM / SSB: everything before the first per-sample recursion.
//   AM (audio AGC):  pre[i] = |x[i]|                         (volk_32fc_magnitude_32f, am.h:120)
//   SSB:             pre[i] = Re{ x[i] * e^{j(phi2 + i*theta2)} }   (ssb.h:79-88: second translation + ComplexToReal)
struct PreJob {
    int mode, n;
    const float2* in;
    float* out;
    double theta2, phi2;
};
__device__ __forceinline__ void vfo_demod_pre_body(const KIdx bid, const KIdx gdim, const PreJob* __restrict__ jobs) {
    const PreJob& job = jobs[bid.y];
    for (int i = bid.x * blockDim.x + threadIdx.x; i < job.n; i += gdim.x * blockDim.x) {
        const float2 x = global_load_f32x2(job.in, i);  // (explicit GLOBAL accesses: FLAT ones as a tick role)
        if (job.mode == 2) { global_store_f32_boff(job.out, (unsigned)i * 4u, cabs_ref(x)); }
        else {
            float sn, cs;
            turn_sincos(fma((double)i, job.theta2, job.phi2), sn, cs);
            global_store_f32_boff(job.out, (unsigned)i * 4u, cmul_re(x, cs, sn));
        }
    }
}
__global__ __launch_bounds__(256) void vfo_demod_pre_kernel(const PreJob* __restrict__ jobs) { vfo_demod_pre_body(kidx(blockIdx), kidx(gridDim), jobs); }

struct SeqJob {
    int mode;  // 2 AM, 3/4/5 SSB family, 6 CW (the SSB arithmetic with the tone as its translation)
    int n;
    const float2* in;  // complex IF samples of this push (AM carrier-AGC mode only)
    float* pre;        // real samples from vfo_demod_pre_kernel; AM overwrites them in place with the low-pass input
    float* out;        // SSB: stereo float2 output
    AgcState* agc;     // persistent (device)
    AgcState* carrier_agc;
    float* dc_offset;  // persistent
    float dc_rate;
    int carrier_mode;
    // reference blocks inside this push (cumulative sample counts; nullptr: the push is one block).  loop::AGC's look-ahead on
    // clipping scans to the end of the CURRENT BLOCK (agc.h:91-104), so its result depends on how the reference cut the stream.
    const int* bounds;
    int nb;
};

__device__ __forceinline__ float agc_gain(AgcState& a, float inAmp) {
    float gain;
    if (inAmp != 0.0f) {
        a.amp = (inAmp > a.amp) ? ((a.amp * a.inv_attack) + (inAmp * a.attack)) : ((a.amp * a.inv_decay) + (inAmp * a.decay));
        const float g = a.set_point / a.amp;
        gain = (a.max_gain < g) ? a.max_gain : g;
    }
    else {
        gain = 1.0f;
    }
    return gain;
}

// loop::AGC's amplitude tracker alone (agc.h:79-83): the part of the recursion that is really sequential.  The gain — a division per
// sample — depends on it but nothing depends on the gain, so it is taken out of the chain and evaluated for 64 samples at once.
__device__ __forceinline__ float agc_track(float amp, float inAmp, const AgcState& a) {
    if (inAmp != 0.0f) {
        const bool up = inAmp > amp;
        const float c1 = up ? a.inv_attack : a.inv_decay, c2 = up ? a.attack : a.decay;
        amp = (amp * c1) + (inAmp * c2);
    }
    return amp;
}
__device__ __forceinline__ float agc_gain_of(float amp, float inAmp, const AgcState& a) {
    if (inAmp == 0.0f) { return 1.0f; }
    const float g = a.set_point / amp;
    return (a.max_gain < g) ? a.max_gain : g;
}

// One WAVEFRONT per VFO: only the recursions (DC blocker, AGC) are left here.  The lanes fetch 64 consecutive samples with one
// coalesced load; every lane then evaluates the same (uniform) recursion, taking sample i from lane i with v_readlane — a
// one-work-item loop over global memory pays ~1 us of load latency per sample.  The AGC's look-ahead to the end of the push
// (agc.h:91-104) is a wave-wide max reduction where it is a plain maximum, and the same chunked loop where it has to re-run the
// DC blocker forward (AM, audio AGC).
__device__ __forceinline__ void vfo_sequential_body(const KIdx bid, const SeqJob* __restrict__ jobs, int njobs) {
    const int id = bid.x;
    if (id >= njobs) { return; }
    const SeqJob job = jobs[id];
    const int lane = threadIdx.x;
    const int nblk = job.bounds ? job.nb : 1;
    if (job.mode == 2) {
        AgcState agc = *job.agc;
        AgcState cagc = *job.carrier_agc;
        float off = *job.dc_offset;
        int blk_lo = 0;
        for (int blk = 0; blk < nblk; blk++) {
        const int n = job.bounds ? job.bounds[blk] : job.n;  // end of this reference block
        for (int base = blk_lo; base < n; base += 64) {
            const int cnt = (n - base < 64) ? n - base : 64;
            float2 xin = make_float2(0.0f, 0.0f);
            float pv = 0.0f;
            if (lane < cnt) {
                if (job.carrier_mode) { xin = job.in[base + lane]; }
                else { pv = job.pre[base + lane]; }
            }
            const float amp_l = sqrtf((xin.x * xin.x) + (xin.y * xin.y));  // carrier mode: |x| of this lane's sample
            float outv = 0.0f;
            if (job.carrier_mode) {
                // carrier AGC on the complex IF (am.h:103-106), then envelope and DC blocker: sample by sample
                for (int i = 0; i < cnt; i++) {
                    float2 x = make_float2(wave_bcast(xin.x, i), wave_bcast(xin.y, i));
                    const float inAmp = wave_bcast(amp_l, i);
                    float gain = agc_gain(cagc, inAmp);
                    if (inAmp * gain > cagc.max_output_amp) {
                        float m = (lane >= i && lane < cnt) ? amp_l : 0.0f;  // rest of this chunk, then the rest of the block
                        for (int b2 = base + 64 + lane; b2 < n; b2 += 64) {
                            const float2 y = job.in[b2];
                            const float a = sqrtf((y.x * y.x) + (y.y * y.y));
                            if (a > m) { m = a; }
                        }
                        cagc.amp = wave_max(m);
                        const float g = cagc.set_point / cagc.amp;
                        gain = (cagc.max_gain < g) ? cagc.max_gain : g;
                    }
                    x.x = x.x * gain;
                    x.y = x.y * gain;
                    const float mag = sqrtf((x.x * x.x) + (x.y * x.y));
                    const float v = mag - off;
                    off += v * job.dc_rate;
                    if (lane == i) { outv = v; }
                }
            }
            else {
                // envelope (already in `pre`) -> DC blocker -> audio AGC.  Sequential per chunk: only the DC blocker and the AGC's amplitude
                // tracker (lane i keeps v, the tracker and the blocker's offset after sample i); gains and the clip test in one parallel step.
                // A clip is handled at its sample as the reference does: the look-ahead needs the not-yet-computed future samples of the same
                // recursion, so it re-runs the DC blocker forward to the end of the BLOCK from the state behind that sample (exactly what
                // the reference's in-place buffer holds at that moment), and the scan restarts behind it.
                int i0 = 0;
                while (i0 < cnt) {
                    float o = off, amp = agc.amp, my_v = 0.0f, my_amp = 0.0f, my_off = 0.0f;
                    for (int i = i0; i < cnt; i++) {
                        const float v = wave_bcast(pv, i) - o;
                        o += v * job.dc_rate;
                        amp = agc_track(amp, fabsf(v), agc);
                        if (lane == i) {
                            my_v = v;
                            my_amp = amp;
                            my_off = o;
                        }
                    }
                    const bool mine = lane >= i0 && lane < cnt;
                    const float a_l = fabsf(my_v);
                    const float g_l = mine ? agc_gain_of(my_amp, a_l, agc) : 1.0f;
                    const int f = wave_first(mine && (a_l * g_l > agc.max_output_amp));
                    if (mine && lane < f) { outv = my_v * g_l; }
                    if (f >= 64) {
                        off = o;
                        agc.amp = amp;
                        break;
                    }
                    float maxAmp = wave_bcast(a_l, f);
                    float o2 = wave_bcast(my_off, f);
                    off = o2;
                    for (int jn = f + 1; jn < cnt; jn++) {
                        const float v2 = wave_bcast(pv, jn) - o2;
                        o2 += v2 * job.dc_rate;
                        const float a2 = fabsf(v2);
                        if (a2 > maxAmp) { maxAmp = a2; }
                    }
                    for (int b2 = base + 64; b2 < n; b2 += 64) {
                        const int c2 = (n - b2 < 64) ? n - b2 : 64;
                        const float q = (lane < c2) ? job.pre[b2 + lane] : 0.0f;
                        for (int jn = 0; jn < c2; jn++) {
                            const float v2 = wave_bcast(q, jn) - o2;
                            o2 += v2 * job.dc_rate;
                            const float a2 = fabsf(v2);
                            if (a2 > maxAmp) { maxAmp = a2; }
                        }
                    }
                    agc.amp = maxAmp;
                    const float g = agc.set_point / agc.amp;
                    const float gain = (agc.max_gain < g) ? agc.max_gain : g;
                    if (lane == f) { outv = my_v * gain; }
                    i0 = f + 1;
                }
            }
            if (lane < cnt) { job.pre[base + lane] = outv; }
        }
        blk_lo = n;
        }
        if (lane == 0) {
            *job.agc = agc;
            *job.carrier_agc = cagc;
            *job.dc_offset = off;
        }
    }
    else {
        AgcState agc = *job.agc;
        float2* out = reinterpret_cast<float2*>(job.out);
        int blk_lo = 0;
        for (int blk = 0; blk < nblk; blk++) {
        const int n = job.bounds ? job.bounds[blk] : job.n;
        for (int base = blk_lo; base < n; base += 64) {
            const int cnt = (n - base < 64) ? n - base : 64;
            const float pv = (lane < cnt) ? job.pre[base + lane] : 0.0f;
            const float a_l = fabsf(pv);
            float outv = 0.0f;
            // Chunk of 64 samples: the amplitude tracker runs sequentially (uniform, ~10 instructions per sample), lane i keeps the value
            // after sample i; gains and the clip test are then one parallel step.  A clip (rare: the start of a burst) is handled at its
            // sample exactly as the reference does — amp = maximum over the rest of the BLOCK — and the scan restarts behind it.
            int i0 = 0;
            while (i0 < cnt) {
                float amp = agc.amp, my_amp = 0.0f;
                for (int i = i0; i < cnt; i++) {
                    amp = agc_track(amp, wave_bcast(a_l, i), agc);
                    if (lane == i) { my_amp = amp; }
                }
                const bool mine = lane >= i0 && lane < cnt;
                const float g_l = mine ? agc_gain_of(my_amp, a_l, agc) : 1.0f;
                const int f = wave_first(mine && (a_l * g_l > agc.max_output_amp));
                if (mine && lane < f) { outv = pv * g_l; }
                if (f >= 64) {
                    agc.amp = amp;
                    break;
                }
                float m = (lane >= f && lane < cnt) ? a_l : 0.0f;  // rest of this chunk, then the rest of the block
                for (int b2 = base + 64 + lane; b2 < n; b2 += 64) {
                    const float a2 = fabsf(job.pre[b2]);
                    if (a2 > m) { m = a2; }
                }
                agc.amp = wave_max(m);
                const float g = agc.set_point / agc.amp;
                const float gain = (agc.max_gain < g) ? agc.max_gain : g;
                if (lane == f) { outv = pv * gain; }
                i0 = f + 1;
            }
            if (lane < cnt) { out[base + lane] = make_float2(outv, outv); }
        }
        blk_lo = n;
        }
        if (lane == 0) { *job.agc = agc; }
    }
}
__global__ __launch_bounds__(64) void vfo_sequential_kernel(const SeqJob* __restrict__ jobs, int njobs) { vfo_sequential_body(kidx(blockIdx), jobs, njobs); }

}  // namespace sdrpp_k
