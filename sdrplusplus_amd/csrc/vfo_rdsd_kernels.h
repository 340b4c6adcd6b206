// The RDS demodulator behind the WFM demodulator's RDS branch (or behind any 5 kS/s RAW VFO): AGC, two Costas loops around a complex band-pass, Mueller-Mueller
// clock recovery, slicer and differential decoder — soft symbols and decoded bits.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <sdrpp_gfx950.h>

namespace sdrpp_k {

// =====================================================================================================================
// RDSDemod::process (decoder_modules/radio/src/rds_demod.h:64-74), per input sample x[i] and per symbol:
//     a[i]  = x[i] * gain;  amp = sqrt(a.re^2 + a.im^2);  gain += (setPoint - amp) * rate, clamped from above       (loop/fast_agc.h:60-79)
//     c[i]  = a[i] * phasor(-phase1);  advance1(clamp(c.re * c.im, -1, 1))                                          (loop/costas.h:17-45, phase_control_loop.h:58-85)
//     f[i]  = sum_k c[i - (K-1) + k] * h[k]                     (FIR<complex_t, complex_t>: volk_32fc_x2_dot_prod_32fc in the generic order, k ascending)
//     r[i]  = (f[i] * phasor(-phase2)).re;  advance2(clamp(re * im, -1, 1))                                         (the second Costas<2>, then ComplexToReal)
//     MM<float>::process over r (clock_recovery/mm.h:100-156), as vfo_sym_kernels.h restates it; per symbol b = soft > 0 (binary_slicer.h),
//     bit = (b - last + 2) % 2, last = b                                                                            (differential_decoder.h:41-46)
// in float throughout, every operation the reference's, in its order, rounded on its own (the library is built without contraction).
// ONE WAVEFRONT PER CHANNEL AND BLOCK (WK_RDS_DEMOD): three recursions and a long filter alternate, so the wavefront that owns a channel keeps everything
// between them in its share of the role's LDS and walks the block in chunks of 64 samples:
//   load     lane i holds sample i; the next chunk's load is in flight while this one is walked
//   serial 1 AGC and first loop, uniform: the sample comes out of lane i's register (v_readlane: no memory wait on the chain); the result goes behind the
//            K - 1 carried values of the filter's window in LDS
//   parallel lane j computes filter output j over the window, taps from scalar loads; the window then moves down by the chunk
//   serial 2 second loop, uniform, its real parts behind the T - 1 carried values of MM's work buffer in LDS; then MM's walk over the chunk: `offset` counts
//            from the chunk's first sample exactly as the reference's counts from its block's first (the reference is causal per sample: any cut gives
//            the same bits), followed by `offset -= chunk` and the T - 1 newest values moved to the front
// PUSH ENDS cut nothing but the COUNT: a symbol belongs to the push its start lies in, so the walk of a chunk stops at every push end inside it, stores that
// push's count, and goes on.
// INTERPOLATOR BANK: the row of the symbol's phase is read through the cache with scalar loads (the phase index is wave-uniform: one s_load of T floats), as the
// pager loop reads it with vector loads.  The alternative — the bank in 16 registers per lane, the row fetched by lane index — holds exactly the reference's
// 128 x 8 bank and nothing larger, while the description admits up to 1024 x 16; a second code path for one shape was not worth its registers in a role whose
// occupancy the FFT tick depends on.  A symbol comes every 4.2 samples; the row's read lies on the symbol's chain (an L2 hit at worst, the bank is 4 KB).
// MM's symbol step is a second copy of vfo_sym_loop_body's, not a shared function: that one reads its row from global memory per lane, this one from LDS, uniform;
// a shared function would have had to be proven to leave the pager's machine code alone.
// BOUNDED LOOPS: the reference's clampPhase is `while (phase > max) phase -= delta`.  The host admits only loops with max(|min_freq|, |max_freq|) + |alpha| <=
// 2 pi (rdsd_apply), so one conditional subtraction and one conditional addition are that loop exactly; they are selects.  MM's step is clamped and its stores
// are bounded by the outputs' capacity as in vfo_sym_loop_body.  Samples that are not numbers give unspecified values; every trip count depends on n alone.
// STATE, one device array per channel, updated in place (SDRPP_RDSD_STATE_HEAD words, then the filter's line of K - 1 complex values, then MM's T - 1):
//     [0] gain  [1] phase1  [2] freq1  [3] phase2  [4] freq2  [5] MM phase  [6] MM freq  [7] lastOut  [8] offset (int)  [9] decoder's last (int)
// =====================================================================================================================
#ifndef SDRPP_WAVE_LDS_FLOATS
#error "a part of vfo_ifchain_kernels.h, the role's header: include that one"
#endif
#define SDRPP_RDSD_CHUNK 64
#define SDRPP_RDSD_MAX_TAPS 256           // complex taps: the window of (chunk + K - 1) complex values and MM's work buffer must fit the stride (vfo_ifchain_kernels.h)
#define SDRPP_RDSD_WIN_FLOATS (2 * (SDRPP_RDSD_CHUNK + SDRPP_RDSD_MAX_TAPS - 1))
#define SDRPP_RDSD_MM_FLOATS (SDRPP_RDSD_CHUNK + SDRPP_SYM_MAX_INTERP_TAPS - 1)
#define SDRPP_RDSD_LDS_FLOATS (SDRPP_RDSD_WIN_FLOATS + 2 + SDRPP_RDSD_MM_FLOATS)
#define SDRPP_RDSD_STATE_HEAD 16

struct RdsdJob {
    const float2* x;      // the block's input: complex samples at the demodulator's rate
    float* soft;          // the block's symbols, all pushes of a launch group in one piece
    uint8_t* bits;
    int* counts;          // symbols per push
    float* state;         // persistent (device): the layout above
    const float* taps;    // K complex taps, interleaved, natural order
    const float* bank;    // phases x T, phase-major
    const int* ends;      // a launch group: the cumulative push ends at this stream's rate (nullptr: one push, n)
    float set_point, max_gain, rate;
    float alpha1, beta1, min_freq1, max_freq1;
    float alpha2, beta2, min_freq2, max_freq2;
    float mu_gain, omega_gain, min_omega, max_omega;
    int K, T, phases;
    int n, npush;
    int cap;              // symbols soft / bits have room for
    int pad;
};
static_assert(sizeof(RdsdJob) % 8 == 0, "records lie in an array");

// PhaseControlLoop<float>::advance with phase limits +-FL_M_PI (pll.h:22)
__device__ __forceinline__ void rdsd_advance(float err, float alpha, float beta, float min_freq, float max_freq, float& phase, float& freq) {
    const float FL_PI = 3.1415926535f, TWO_PI = FL_PI - (-FL_PI);  // phase_control_loop.h:28: phaseDelta = maxPhase - minPhase
    freq = freq + (beta * err);
    freq = (freq > max_freq) ? max_freq : ((freq < min_freq) ? min_freq : freq);
    phase = phase + (freq + (alpha * err));
    phase = (phase > FL_PI) ? phase - TWO_PI : phase;
    phase = (phase < -FL_PI) ? phase + TWO_PI : phase;
}
// in * phasor(-phase): complex_t::operator*, every product in place (types.h:23-25)
__device__ __forceinline__ float2 rdsd_derotate(float re, float im, float phase) {
    const float vr = cosf(-phase), vi = sinf(-phase);
    return make_float2((re * vr) - (im * vi), (im * vr) + (re * vi));
}
// Costas<2>::errorFunction: std::clamp(re * im, -1, 1)
__device__ __forceinline__ float rdsd_error(float2 v) {
    const float e = v.x * v.y;
    return (e < -1.0f) ? -1.0f : ((1.0f < e) ? 1.0f : e);
}
__device__ __forceinline__ float rdsd_step(float x) { return (x > 0.0f) ? 1.0f : -1.0f; }  // math/step.h

__device__ __forceinline__ void vfo_rdsd_body(const RdsdJob& job, float* smem) {
    const int lane = threadIdx.x & 63, wv = (int)threadIdx.x >> 6;
    float2* W = reinterpret_cast<float2*>(smem + wv * SDRPP_WAVE_LDS_FLOATS);  // [K - 1 carried][chunk]
    float* M = smem + wv * SDRPP_WAVE_LDS_FLOATS + SDRPP_RDSD_WIN_FLOATS + 2;  // [T - 1 carried][chunk]
    const int K = min(max(job.K, 1), SDRPP_RDSD_MAX_TAPS), T = min(max(job.T, 1), SDRPP_SYM_MAX_INTERP_TAPS), n = job.n;
    const UniformF32 taps = as_uniform(job.taps), bank = as_uniform(job.bank);
    const float* line = job.state + SDRPP_RDSD_STATE_HEAD;
    const float* mline = line + 2 * (K - 1);
    float gain = global_load_f32(job.state, 0);
    float ph1 = global_load_f32(job.state, 1), fr1 = global_load_f32(job.state, 2);
    float ph2 = global_load_f32(job.state, 3), fr2 = global_load_f32(job.state, 4);
    float mph = global_load_f32(job.state, 5), mfr = global_load_f32(job.state, 6), last = global_load_f32(job.state, 7);
    int off = __float_as_int(global_load_f32(job.state, 8));
    int dlast = __float_as_int(global_load_f32(job.state, 9));
    for (int p = lane; p < K - 1; p += 64) { W[p] = make_float2(global_load_f32(line, 2 * p), global_load_f32(line, 2 * p + 1)); }
    if (lane < T - 1) { M[lane] = global_load_f32(mline, lane); }
    wave_sync();
    const float fphases = (float)job.phases;
    int nsym = 0, q = 0, cnt_q = 0;
    int end_q = (job.ends && job.npush > 0) ? global_load_i32(job.ends, 0) : n;
    float2 xnext = (lane < n) ? global_load_f32x2(job.x, lane) : make_float2(0.0f, 0.0f);
    for (int base = 0; base < n; base += SDRPP_RDSD_CHUNK) {
        const int cnt = min(SDRPP_RDSD_CHUNK, n - base);
        const float2 x = xnext;
        if (base + SDRPP_RDSD_CHUNK + lane < n) { xnext = global_load_f32x2(job.x, base + SDRPP_RDSD_CHUNK + lane); }  // the next chunk travels while this one is walked
        // ---- serial pass 1: AGC, first loop ----
        float2 mine = make_float2(0.0f, 0.0f);
        for (int i = 0; i < cnt; i++) {
            const float are = wave_bcast(x.x, i) * gain, aim = wave_bcast(x.y, i) * gain;
            const float amp = sqrtf((are * are) + (aim * aim));
            gain = gain + ((job.set_point - amp) * job.rate);
            gain = (gain > job.max_gain) ? job.max_gain : gain;
            const float2 c = rdsd_derotate(are, aim, ph1);
            rdsd_advance(rdsd_error(c), job.alpha1, job.beta1, job.min_freq1, job.max_freq1, ph1, fr1);
            if (lane == i) { mine = c; }
        }
        if (lane < cnt) { W[(K - 1) + lane] = mine; }
        wave_sync();
        // ---- parallel pass: filter output j in lane j (lanes past the chunk's end read what an earlier chunk left in the window: never used) ----
        float fre = 0.0f, fim = 0.0f;
        for (int k = 0; k < K; k++) {
            const float2 a = W[lane + k];
            const float hr = taps[2 * k], hi = taps[2 * k + 1];
            fre = fre + ((a.x * hr) - (a.y * hi));
            fim = fim + ((a.x * hi) + (a.y * hr));
        }
        // the window moves down by the chunk: K - 1 values, 64 at a time (a round reads what it and later rounds have not yet overwritten)
        for (int p0 = 0; p0 < K - 1; p0 += 64) {
            const int p = p0 + lane;
            float2 v = make_float2(0.0f, 0.0f);
            if (p < K - 1) { v = W[p + cnt]; }
            wave_sync();
            if (p < K - 1) { W[p] = v; }
            wave_sync();
        }
        // ---- serial pass 2: second loop, its real part into MM's work buffer ----
        float mre = 0.0f;
        for (int i = 0; i < cnt; i++) {
            const float2 c = rdsd_derotate(wave_bcast(fre, i), wave_bcast(fim, i), ph2);
            rdsd_advance(rdsd_error(c), job.alpha2, job.beta2, job.min_freq2, job.max_freq2, ph2, fr2);
            if (lane == i) { mre = c.x; }
        }
        if (lane < cnt) { M[(T - 1) + lane] = mre; }
        wave_sync();
        // ---- MM's walk over the chunk, push by push ----
        for (;;) {
            const int lim = min(end_q - base, cnt);  // symbols that start in front of it belong to push q
            while (off < lim && nsym < job.cap) {
                int p = (int)floorf(mph * fphases);
                p = wave_uniform(min(max(p, 0), job.phases - 1));
                float out = 0.0f;
                for (int k = 0; k < T; k++) { out = out + (M[off + k] * bank[p * T + k]); }
                const int b = (out > 0.0f) ? 1 : 0;
                if (lane == 0) {
                    global_store_f32_boff(job.soft, (unsigned)nsym * 4u, out);
                    job.bits[nsym] = (uint8_t)((b - dlast + 2) % 2);
                }
                dlast = b;
                nsym++;
                cnt_q++;
                float error = (rdsd_step(last) * out) - (last * rdsd_step(out));
                last = out;
                if (error > 1.0f) { error = 1.0f; }
                if (error < -1.0f) { error = -1.0f; }
                mfr = mfr + (job.omega_gain * error);
                if (mfr > job.max_omega) { mfr = job.max_omega; }
                else if (mfr < job.min_omega) { mfr = job.min_omega; }
                mph = mph + (mfr + (job.mu_gain * error));
                const float delta = floorf(mph);
                // (offset += delta: exact; a description rdsd_apply has taken steps 1 .. SDRPP_SYM_MAX_STEP + 1 samples — the bounds only keep samples that are
                // not numbers from stalling the walk or carrying it away)
                int step = (int)delta;
                step = (step >= 1) ? step : 1;
                step = (step <= SDRPP_SYM_MAX_STEP + 2) ? step : SDRPP_SYM_MAX_STEP + 2;
                off += step;
                mph = mph - delta;
            }
            if (end_q > base + cnt || q >= job.npush) { break; }
            if (lane == 0) { global_store_u32(job.counts, q, (unsigned)cnt_q); }  // push q ends inside this chunk
            cnt_q = 0;
            q++;
            if (q >= job.npush) { break; }
            end_q = job.ends ? global_load_i32(job.ends, q) : n;
        }
        off = ((off > cnt) ? off : cnt) - cnt;
        float mv = 0.0f;
        if (lane < T - 1) { mv = M[cnt + lane]; }
        wave_sync();
        if (lane < T - 1) { M[lane] = mv; }
        wave_sync();
    }
    // pushes that end where no chunk does (a block without samples; empty pushes at its end)
    for (; q < job.npush; q++) {
        if (lane == 0) { global_store_u32(job.counts, q, (unsigned)cnt_q); }
        cnt_q = 0;
    }
    float* sline = job.state + SDRPP_RDSD_STATE_HEAD;
    for (int p = lane; p < K - 1; p += 64) { global_store_f32x2_boff(sline, (unsigned)p * 8u, W[p]); }
    if (lane < T - 1) { global_store_f32_boff(sline, (unsigned)(2 * (K - 1) + lane) * 4u, M[lane]); }
    if (lane == 0) {
        global_store_f32_boff(job.state, 0u, gain);
        global_store_f32_boff(job.state, 4u, ph1);
        global_store_f32_boff(job.state, 8u, fr1);
        global_store_f32_boff(job.state, 12u, ph2);
        global_store_f32_boff(job.state, 16u, fr2);
        global_store_f32_boff(job.state, 20u, mph);
        global_store_f32_boff(job.state, 24u, mfr);
        global_store_f32_boff(job.state, 28u, last);
        global_store_f32_boff(job.state, 32u, __int_as_float(off));
        global_store_f32_boff(job.state, 36u, __int_as_float(dlast));
    }
}

// (a call, not inlined, as the other branches' bodies are: the role's own code and the tick kernel's register allocation stay what they are)
__device__ __attribute__((noinline)) void vfo_rdsd_call(const RdsdJob* j, float* smem) { vfo_rdsd_body(wave_uniform_job(j), smem); }

}  // namespace sdrpp_k
