// The Meteor QPSK demodulator on a RAW VFO: root-raised-cosine FIR, AGC, QPSK Costas loop, optional OQPSK delay, complex Mueller-Mueller clock recovery —
// complex soft symbols and their int8 pairs.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <sdrpp_gfx950.h>
#include "vfo_stream.h"

namespace sdrpp_k {

// =====================================================================================================================
// dsp::demod::Meteor::process (decoder_modules/meteor_demodulator/src/meteor_demod.h:150-167), per input sample x[i] and per symbol:
//     f[i]  = sum_k x[i - (K-1) + k] * h[k]             FIR<complex_t, float>: volk_32fc_32f_dot_prod_32fc in the generic order — re and im each accumulated
//                                                        sequentially, k ascending, every product and sum rounded apart
//     a[i]  = f[i] * gain;  amp = sqrt(a.re^2 + a.im^2);  gain += (setPoint - amp) * rate, clamped from above       (loop/fast_agc.h:60-79)
//     c[i]  = a[i] * phasor(-phase);  advance(error(c[i]))                                                          (meteor_costas.h:24-56, phase_control_loop.h:58-85)
//             error = clamp(step(c.re) * c.im - step(c.im) * c.re, -1, 1), or the four-phase rule of the "broken modulation" (qpsk_error_broken)
//     oqpsk:  tmp = c.im;  c.im = lastI;  lastI = tmp                                                                (meteor_demod.h:155-162)
//     MM<complex_t>::process over c (clock_recovery/mm.h:100-156): while offset < count: interpolate re and im at `offset` (volk_32fc_32f_dot_prod_32fc),
//             p2 <- p1 <- p0 <- out;  c2 <- c1 <- c0 <- step(out);  error = ((p0 - p2) * conj(c1) - (c0 - c2) * conj(p1)).re, clamped;  pcl.advance;
//             offset += floorf(phase)
//     and the module's sink (main.cpp:193-201): int8 = clamp((int)(v * 84), -127, 127) of re and of im
// in float throughout, every operation the reference's, in its order, rounded on its own (the library is built without contraction).
// THE LONG FILTER STANDS IN FRONT OF EVERY RECURSION: it is feed-forward on the raw stream, so it is spread over many wavefronts and is not interleaved with a
// serial pass.  Two kinds of the wavefront-job role (vfo_ifchain_kernels.h), a level each:
//   front  (WK_QPSK_FRONT) the filter: one record per VFO and block, a wave job per segment of SDRPP_QPSK_SEG samples (its first sample in WaveJob::arg, as
//          FMIF is filed), tiled through the wavefront's share of the role's LDS: the window of a tile (SDRPP_QPSK_TILE + K - 1 complex values), two outputs per
//          lane, taps from scalar loads.  Its output goes to a per-channel buffer of the stream's capacity.
//   loop   (WK_QPSK_LOOP) everything sequential, one level behind: ONE wavefront per channel and block, in chunks of 64 filter outputs in the form of
//          vfo_rdsd_body — lane i holds output i (the next chunk's load in flight), the serial pass is uniform over the wavefront and reads sample i out of lane
//          i's register (v_readlane), its result goes behind the T - 1 carried complex values of MM's work buffer in LDS; then MM's walk over the chunk.
//          `offset` counts from the chunk's first sample exactly as the reference's counts from its block's first (the reference is causal per sample: any cut
//          gives the same symbols).
// THE DEMODULATOR'S STATE IS ITS OWN (switched off it freezes while the VFO's stream moves on: nothing here reads the feed's history).
//   front: `lines`, two sides of K - 1 complex inputs each (what FIR::buffer holds), newest last: a block reads side `cur` and the job that holds the block's last
//          sample writes the other; the host flips them per block that has samples — the segments of a block all read the old side while one of them writes
//   loop:  one device array, updated in place (SDRPP_QPSK_STATE_HEAD words, then MM's T - 1 complex samples):
//          [0] gain  [1] loop phase  [2] loop freq  [3] lastI  [4] MM phase  [5] MM freq  [6] offset (int)  [8..13] _p_0T _p_1T _p_2T  [14..19] _c_0T _c_1T _c_2T
// PUSH ENDS cut nothing but the COUNT, as in vfo_rdsd_body: a symbol belongs to the push its start lies in.
// INT8 PAIRS: (int8)clamp((int)(v * soft_scale), -127, 127), the conversion truncating towards zero; the clamp is done in float first, so that the conversion is
// defined for every input (the reference's is not), and a NaN gives 0.  Two symbols make a word: the pair of an even symbol waits in a register for its
// neighbour and both leave in one 32-bit vector store; an odd count's last pair leaves as a 16-bit store.
// BOUNDED LOOPS, as vfo_rdsd_kernels.h states them: the host admits only a loop with max(|min_freq|, |max_freq|) + |alpha| <= 2 pi and |init_phase| <= pi
// (qpsk_apply), so the phase wrap is two selects; MM's step is clamped to 1 .. SDRPP_SYM_MAX_STEP + 2 and the stores are bounded by the outputs' capacity.
// Samples that are not numbers give unspecified values; every trip count depends on n alone.
// =====================================================================================================================
#ifndef SDRPP_WAVE_LDS_FLOATS
#error "a part of vfo_ifchain_kernels.h, the role's header: include that one"
#endif
#define SDRPP_QPSK_SEG 512               // front: samples per wave job
#define SDRPP_QPSK_TILE 128              // front: outputs per tile (two per lane)
#define SDRPP_QPSK_MAX_TAPS 256          // real taps: the window of (tile + K - 1) complex values must fit the stride (vfo_ifchain_kernels.h)
#define SDRPP_QPSK_WIN (SDRPP_QPSK_TILE + SDRPP_QPSK_MAX_TAPS - 1)
#define SDRPP_QPSK_FRONT_LDS_FLOATS (2 * SDRPP_QPSK_WIN)
#define SDRPP_QPSK_CHUNK 64
#define SDRPP_QPSK_LOOP_LDS_FLOATS (2 * (SDRPP_QPSK_CHUNK + SDRPP_SYM_MAX_INTERP_TAPS - 1))  // MM's work buffer; the serial pass stages nothing else (its values leave lane registers)
#define SDRPP_QPSK_STATE_HEAD 24

// One record per VFO and block (WK_QPSK_FRONT); a wave job is one segment of it, its first sample in WaveJob::arg.
struct QpskFrontJob {
    const float2* x;      // the stream a demodulator would read: this block's samples only
    float* lines;         // the two sides, 2 K floats each: K - 1 complex inputs, newest last (one complex spare)
    float2* buf;          // f[0 .. n)
    const float* taps;    // K real taps, natural order
    int n, cur;
    int K, pad;
};
static_assert(sizeof(QpskFrontJob) % 8 == 0, "records lie in an array");

__device__ __forceinline__ void vfo_qpsk_front_body(const QpskFrontJob& job, int lo, float* smem) {
    const int lane = threadIdx.x & 63, wv = (int)threadIdx.x >> 6;
    float2* W = reinterpret_cast<float2*>(smem + wv * SDRPP_WAVE_LDS_FLOATS);
    const int K = min(max(job.K, 1), SDRPP_QPSK_MAX_TAPS), n = job.n;
    const int hi = min(lo + SDRPP_QPSK_SEG, n);
    const UniformF32 taps = as_uniform(job.taps);
    const float* line = job.lines + job.cur * (2 * K);
    float* line_new = job.lines + (job.cur ^ 1) * (2 * K);
    const StreamIn in{ reinterpret_cast<const float*>(job.x), line, K - 1, n };  // (the line is the stream's history: sample -1 is its last element)
#pragma unroll 1
    for (int t0 = lo; t0 < hi; t0 += SDRPP_QPSK_TILE) {
        const int cnt = min(SDRPP_QPSK_TILE, hi - t0);
        const int base = t0 - (K - 1);   // stream index of window element 0 (>= -(K - 1): inside the line)
        const int nvalid = cnt + K - 1;  // window elements
        // W[p] = x[base + p], every load of the window in flight before the first store; zero behind the tile's last sample
        constexpr int R = (SDRPP_QPSK_WIN + 63) / 64;
        float2 pf[R];
#pragma unroll
        for (int q = 0; q < R; q++) {
            const int p = q * 64 + lane;
            pf[q] = make_float2(0.0f, 0.0f);
            if (q * 64 < nvalid) { pf[q] = stream_load2_nb(in, base + p, p < nvalid); }  // (wave-uniform: a short filter's window takes fewer rounds)
        }
#pragma unroll
        for (int q = 0; q < R; q++) {
            const int p = q * 64 + lane;
            if (q * 64 < nvalid && p < SDRPP_QPSK_WIN) { W[p] = pf[q]; }
        }
        wave_sync();
        float re0 = 0.0f, im0 = 0.0f, re1 = 0.0f, im1 = 0.0f;
        const float2* w = W + lane;
        for (int k = 0; k < K; k++) {
            const float h = taps[k];
            const float2 a0 = w[k], a1 = w[64 + k];
            re0 = re0 + (a0.x * h);
            im0 = im0 + (a0.y * h);
            re1 = re1 + (a1.x * h);
            im1 = im1 + (a1.y * h);
        }
        if (lane < cnt) { global_store_f32x2(job.buf, t0 + lane, make_float2(re0, im0)); }
        if (lane + 64 < cnt) { global_store_f32x2(job.buf, t0 + 64 + lane, make_float2(re1, im1)); }
        wave_sync();  // (the next tile overwrites the window)
    }
    // the job that holds the block's last sample forms the new side: element e is stream sample n - (K - 1) + e — of this block, or (a block shorter than
    // K - 1) element n + e of the old side
    if (hi == n) {
        for (int e = lane; e < K - 1; e += 64) { global_store_f32x2_boff(line_new, (unsigned)e * 8u, stream_load2_nb(in, n - (K - 1) + e)); }
    }
}

// ---- loop: AGC, Costas loop, OQPSK delay, MM's walk ----------------------------------------------------------------------------------------
struct QpskLoopJob {
    const float2* f;      // the front's output of this block
    float2* soft;         // the block's symbols, all pushes of a launch group in one piece
    int8_t* packed;       // two int8 per symbol
    int* counts;          // symbols per push
    float* state;         // persistent (device): the layout above
    const float* bank;    // phases x T, phase-major
    const int* ends;      // a launch group: the cumulative push ends at this stream's rate (nullptr: one push, n)
    float set_point, max_gain, rate;
    float alpha, beta, min_freq, max_freq;
    float mu_gain, omega_gain, min_omega, max_omega;
    float soft_scale;
    int broken, oqpsk;
    int T, phases;
    int n, npush;
    int cap;              // symbols soft / packed have room for
    int pad;
};
static_assert(sizeof(QpskLoopJob) % 8 == 0, "records lie in an array");

__device__ __forceinline__ float qpsk_step(float x) { return (x > 0.0f) ? 1.0f : -1.0f; }  // math/step.h
__device__ __forceinline__ float qpsk_clamp1(float e) { return (e < -1.0f) ? -1.0f : ((1.0f < e) ? 1.0f : e); }  // std::clamp<float>(e, -1, 1)
// MeteorCostas::errorFunction, _broken == false (meteor_costas.h:53)
__device__ __forceinline__ float qpsk_error(float2 v) { return qpsk_clamp1((qpsk_step(v.x) * v.y) - (qpsk_step(v.y) * v.x)); }
// math::normalizePhase (normalize_phase.h): a single conditional each way, `>` above and `<=` below
__device__ __forceinline__ float qpsk_normalize(float d) {
    const float FL_PI = 3.1415926535f;
    return (d > FL_PI) ? d - (2.0f * FL_PI) : ((d <= -FL_PI) ? d + (2.0f * FL_PI) : d);
}
// MeteorCostas::errorFunction, _broken == true (meteor_costas.h:35-51): the phase's distance to the nearest of four constellation phases, in the reference's order
// of comparison (a strictly smaller |dp| replaces), times the amplitude
__device__ __forceinline__ float qpsk_error_broken(float2 v) {
    const float PHASE1 = 0.47439988279190737, PHASE2 = 2.1777839908413044, PHASE3 = 3.8682349942715186, PHASE4 = -0.29067248091319986;
    const float phase = atan2f(v.y, v.x);
    const float dp1 = qpsk_normalize(phase - PHASE1), dp2 = qpsk_normalize(phase - PHASE2), dp3 = qpsk_normalize(phase - PHASE3), dp4 = qpsk_normalize(phase - PHASE4);
    float lowest = dp1;
    lowest = (fabsf(dp2) < fabsf(lowest)) ? dp2 : lowest;
    lowest = (fabsf(dp3) < fabsf(lowest)) ? dp3 : lowest;
    lowest = (fabsf(dp4) < fabsf(lowest)) ? dp4 : lowest;
    return qpsk_clamp1(lowest * sqrtf((v.x * v.x) + (v.y * v.y)));
}
// the module's sink: clamp<int>(v * scale, -127, 127), clamped in float first (the conversion is then defined for every input and truncates towards zero)
__device__ __forceinline__ unsigned qpsk_int8(float v, float scale) {
    float s = v * scale;
    s = (s < -127.0f) ? -127.0f : ((s > 127.0f) ? 127.0f : s);
    s = (s == s) ? s : 0.0f;
    return (unsigned)(int)s & 0xffu;
}

__device__ __forceinline__ void vfo_qpsk_loop_body(const QpskLoopJob& job, float* smem) {
    const int lane = threadIdx.x & 63, wv = (int)threadIdx.x >> 6;
    float2* M = reinterpret_cast<float2*>(smem + wv * SDRPP_WAVE_LDS_FLOATS);  // [T - 1 carried][chunk]
    const int T = min(max(job.T, 1), SDRPP_SYM_MAX_INTERP_TAPS), n = job.n;
    const UniformF32 bank = as_uniform(job.bank);
    const float2* mline = reinterpret_cast<const float2*>(job.state + SDRPP_QPSK_STATE_HEAD);
    float gain = global_load_f32(job.state, 0);
    float ph = global_load_f32(job.state, 1), fr = global_load_f32(job.state, 2), lastI = global_load_f32(job.state, 3);
    float mph = global_load_f32(job.state, 4), mfr = global_load_f32(job.state, 5);
    int off = __float_as_int(global_load_f32(job.state, 6));
    float2 p0 = global_load_f32x2(reinterpret_cast<const float2*>(job.state), 4), p1 = global_load_f32x2(reinterpret_cast<const float2*>(job.state), 5);
    float2 p2 = global_load_f32x2(reinterpret_cast<const float2*>(job.state), 6);
    float2 c0 = global_load_f32x2(reinterpret_cast<const float2*>(job.state), 7), c1 = global_load_f32x2(reinterpret_cast<const float2*>(job.state), 8);
    float2 c2 = global_load_f32x2(reinterpret_cast<const float2*>(job.state), 9);
    if (lane < T - 1) { M[lane] = global_load_f32x2(mline, lane); }
    wave_sync();
    const float fphases = (float)job.phases;
    int nsym = 0, q = 0, cnt_q = 0;
    unsigned pend = 0u;  // the int8 pair of an even symbol, until its neighbour comes
    int end_q = (job.ends && job.npush > 0) ? global_load_i32(job.ends, 0) : n;
    float2 xnext = (lane < n) ? global_load_f32x2(job.f, lane) : make_float2(0.0f, 0.0f);
    for (int base = 0; base < n; base += SDRPP_QPSK_CHUNK) {
        const int cnt = min(SDRPP_QPSK_CHUNK, n - base);
        const float2 x = xnext;
        if (base + SDRPP_QPSK_CHUNK + lane < n) { xnext = global_load_f32x2(job.f, base + SDRPP_QPSK_CHUNK + lane); }  // the next chunk travels while this one is walked
        // ---- serial pass: AGC, loop, OQPSK delay ----
        float2 mine = make_float2(0.0f, 0.0f);
        for (int i = 0; i < cnt; i++) {
            const float are = wave_bcast(x.x, i) * gain, aim = wave_bcast(x.y, i) * gain;
            const float amp = sqrtf((are * are) + (aim * aim));
            gain = gain + ((job.set_point - amp) * job.rate);
            gain = (gain > job.max_gain) ? job.max_gain : gain;
            float2 c = rdsd_derotate(are, aim, ph);
            const float err = job.broken ? qpsk_error_broken(c) : qpsk_error(c);  // (wave-uniform)
            rdsd_advance(err, job.alpha, job.beta, job.min_freq, job.max_freq, ph, fr);
            if (job.oqpsk) {
                const float tmp = c.y;
                c.y = lastI;
                lastI = tmp;
            }
            if (lane == i) { mine = c; }
        }
        if (lane < cnt) { M[(T - 1) + lane] = mine; }
        wave_sync();
        // ---- MM's walk over the chunk, push by push ----
        for (;;) {
            const int lim = min(end_q - base, cnt);  // symbols that start in front of it belong to push q
            while (off < lim && nsym < job.cap) {
                int p = (int)floorf(mph * fphases);
                p = wave_uniform(min(max(p, 0), job.phases - 1));
                float2 out = make_float2(0.0f, 0.0f);
                for (int k = 0; k < T; k++) {
                    const float h = bank[p * T + k];
                    const float2 a = M[off + k];
                    out.x = out.x + (a.x * h);
                    out.y = out.y + (a.y * h);
                }
                const unsigned pair = qpsk_int8(out.x, job.soft_scale) | (qpsk_int8(out.y, job.soft_scale) << 8);
                if (lane == 0) {
                    global_store_f32x2_boff(job.soft, (unsigned)nsym * 8u, out);
                    if (nsym & 1) { global_store_u32(job.packed, nsym >> 1, pend | (pair << 16)); }
                }
                pend = pair;
                nsym++;
                cnt_q++;
                p2 = p1;
                p1 = p0;
                c2 = c1;
                c1 = c0;
                p0 = out;
                c0 = make_float2(qpsk_step(out.x), qpsk_step(out.y));
                // (((p0 - p2) * conj(c1)) - ((c0 - c2) * conj(p1))).re, as complex_t's operators round it (types.h:23-33, :53)
                const float d1x = p0.x - p2.x, d1y = p0.y - p2.y, d2x = c0.x - c2.x, d2y = c0.y - c2.y;
                float error = ((d1x * c1.x) - (d1y * (-c1.y))) - ((d2x * p1.x) - (d2y * (-p1.y)));
                if (error > 1.0f) { error = 1.0f; }
                if (error < -1.0f) { error = -1.0f; }
                mfr = mfr + (job.omega_gain * error);
                if (mfr > job.max_omega) { mfr = job.max_omega; }
                else if (mfr < job.min_omega) { mfr = job.min_omega; }
                mph = mph + (mfr + (job.mu_gain * error));
                const float delta = floorf(mph);
                // (offset += delta: exact; a description qpsk_apply has taken steps 1 .. SDRPP_SYM_MAX_STEP + 1 samples — the bounds only keep samples that are
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
        float2 mv = make_float2(0.0f, 0.0f);
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
    if (lane == 0 && (nsym & 1)) { reinterpret_cast<uint16_t*>(job.packed)[nsym - 1] = (uint16_t)pend; }  // an odd count's last pair
    if (lane < T - 1) { global_store_f32x2_boff(job.state, (unsigned)(SDRPP_QPSK_STATE_HEAD + 2 * lane) * 4u, M[lane]); }
    if (lane == 0) {
        global_store_f32_boff(job.state, 0u, gain);
        global_store_f32_boff(job.state, 4u, ph);
        global_store_f32_boff(job.state, 8u, fr);
        global_store_f32_boff(job.state, 12u, lastI);
        global_store_f32_boff(job.state, 16u, mph);
        global_store_f32_boff(job.state, 20u, mfr);
        global_store_f32_boff(job.state, 24u, __int_as_float(off));
        global_store_f32x2_boff(job.state, 32u, p0);
        global_store_f32x2_boff(job.state, 40u, p1);
        global_store_f32x2_boff(job.state, 48u, p2);
        global_store_f32x2_boff(job.state, 56u, c0);
        global_store_f32x2_boff(job.state, 64u, c1);
        global_store_f32x2_boff(job.state, 72u, c2);
    }
}

// (calls, not inlined, as the other branches' bodies are: the role's own code and the tick kernel's register allocation stay what they are)
__device__ __attribute__((noinline)) void vfo_qpsk_front_call(const QpskFrontJob* j, int lo, float* smem) { vfo_qpsk_front_body(wave_uniform_job(j), lo, smem); }
__device__ __attribute__((noinline)) void vfo_qpsk_loop_call(const QpskLoopJob* j, float* smem) { vfo_qpsk_loop_body(wave_uniform_job(j), smem); }

}  // namespace sdrpp_k
