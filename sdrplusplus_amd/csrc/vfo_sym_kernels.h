// The symbol branch of a RAW VFO: FSK discriminator -> shaping FIR, and Mueller-Mueller clock recovery (soft symbols, sliced bits).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <sdrpp_gfx950.h>
#include "vfo_fir_kernels.h"
#include "vfo_math.h"
#include "vfo_stream.h"

namespace sdrpp_k {

// =====================================================================================================================
// POCSAGDSP (decoder_modules/pager_decoder/src/pocsag/dsp.h:39-45), per IF sample i and per symbol:
//     d[i]  = Quadrature(x[i])                                     (quadrature.h:39-46; fm_phase / normalize_phase, as the audio low-pass takes it)
//     f[i]  = sum_k d[i - (K-1) + k] * h[k]                        (FIR<float, float>: volk_32f_x2_dot_prod_32f in the generic order — product and sum rounded apart)
//     MM<float>::process (clock_recovery/mm.h:100-156): while offset < count: interpolate f at `offset`, error, pcl.advance, offset += floorf(phase)
// Two kinds of the wavefront-job role (vfo_ifchain_kernels.h), a level each:
//   front  (WK_SYM_FRONT) everything in front of the loop: parallel over samples, a wavefront per run of SDRPP_SYM_SEG samples, tiled through its share of the
//          role's LDS as the stereo pilot is
//   loop   (WK_SYM_LOOP) the recursion alone: a LANE per VFO, up to SDRPP_SYM_PACK VFOs per wavefront (SymLoopJob: a run of SymLoopVfo records)
// THE BRANCH'S STATE IS ITS OWN: switched off it freezes while the VFO's stream moves on, so nothing here reads the feed's history.  The front keeps, two
// sides each in one array (a block reads one side and writes the other; the host flips them per block that has samples):
//   line  [K - 1 newest discriminator values, newest last][the discriminator's previous phase]      (what Quadrature::phase and FIR::buffer hold)
//   fh    the T - 1 newest filter outputs, newest last                                                (what MM::buffer holds in front of bufStart)
// and writes the filtered block as MM's work buffer lies: `buf` = [fh: T - 1 values][f[0 .. n)], so that the loop reads one contiguous array.  The job that
// holds the block's last sample forms both new sides from a tile of its own over the last T - 1 outputs (old values spliced in where the block is shorter).
// =====================================================================================================================
#ifndef SDRPP_WAVE_LDS_FLOATS
#error "a part of vfo_ifchain_kernels.h, the role's header: include that one"
#endif
#define SDRPP_SYM_SEG 1024        // samples per front job
#define SDRPP_SYM_TILE 256        // front: outputs per tile (four per lane); its window of tile + K values must fit: K <= SDRPP_SYM_MAX_SHAPE_TAPS
#define SDRPP_SYM_MAX_SHAPE_TAPS 64
#define SDRPP_SYM_MAX_INTERP_TAPS 16
#define SDRPP_SYM_MAX_PHASES 1024
#define SDRPP_SYM_PACK 64         // loop: VFOs per wavefront
#define SDRPP_SYM_MAX_STEP 4096   // loop: |mu_gain| + max_omega at most (sym_apply): offsets stay exact in float and far inside an int

struct SymFrontJob {
    const float2* x;        // the stream a demodulator would read: this block's samples only (nothing in front of the block is read)
    float* lines;           // the two sides, K + T floats each: [line: K floats][fh: T - 1 floats, one spare]; this block reads side `cur` and writes the other
    float* buf;             // [T - 1][n]: fh, then this block's f
    const float* taps;      // K taps, natural order
    int n, cur;             // the block's samples
    int K, T;
    int lo, hi;             // the samples of this job: the one with lo = 0 copies fh in front of the block, the one with hi = n forms the new sides
    float inv_deviation;
    int pad;
};
__device__ __forceinline__ void vfo_sym_front_body(const SymFrontJob& job, float* smem) {
    const int lane = threadIdx.x & 63, wv = (int)threadIdx.x >> 6;
    const int K = job.K, T = job.T, n = job.n;
    float* PH = smem + wv * SDRPP_WAVE_LDS_FLOATS;  // phases, then (in place) the window of d
    const UniformF32 taps = as_uniform(job.taps);
    const StreamIn in{ reinterpret_cast<const float*>(job.x), reinterpret_cast<const float*>(job.x), 0, n };
    const float* line = job.lines + job.cur * (K + T);
    const float* fh = line + K;
    float* line_new = job.lines + (job.cur ^ 1) * (K + T);
    float* fh_new = line_new + K;
    const float prev = global_load_f32(line, K - 1);
    if (job.lo == 0 && lane < T - 1) { global_store_f32_boff(job.buf, (unsigned)lane * 4u, global_load_f32(fh, lane)); }
    // The job's tiles and, for the job that holds the block's last sample, one more over the block's last T - 1 outputs (at least one), which go to the new fh: element e of it is stream
    // sample n - (T - 1) + e — an output of this block, or (a block shorter than T - 1) element n + e of the old side
    const int ntile = (job.hi - job.lo + SDRPP_SYM_TILE - 1) / SDRPP_SYM_TILE;
    const bool tails = job.hi == n && n > 0;
    if (tails && lane < (T - 1) - n) { global_store_f32_boff(fh_new, (unsigned)lane * 4u, global_load_f32(fh, n + lane)); }
#pragma unroll 1
    for (int it = 0; it < ntile + (tails ? 1 : 0); it++) {
        const bool tail = it == ntile;
        // outputs t0 .. t0 + cnt - 1 to dst[dst0 + j] (an index below 0 — the tail tile with T = 1 — is not stored)
        const int cnt = tail ? max(1, min(T - 1, n)) : min(SDRPP_SYM_TILE, job.hi - (job.lo + it * SDRPP_SYM_TILE));
        const int t0 = tail ? n - cnt : job.lo + it * SDRPP_SYM_TILE;
        float* dst = tail ? fh_new : job.buf;
        const int dst0 = tail ? (T - 1) - cnt : (T - 1) + t0;
        const int base = t0 - (K - 1);     // stream index of window element 0
        const int nvalid = cnt + K - 1;    // window elements; PH[p] = phase of stream sample base - 1 + p, p = 0 .. nvalid
        constexpr int U = 4;
        for (int p0 = lane; p0 <= nvalid; p0 += 64 * U) {
            float2 xv[U];
#pragma unroll
            for (int u = 0; u < U; u++) {
                const int p = p0 + 64 * u, i = base - 1 + p;
                xv[u] = stream_load2_nb(in, i, p <= nvalid && i >= 0);
            }
#pragma unroll
            for (int u = 0; u < U; u++) {
                const int p = p0 + 64 * u, i = base - 1 + p;
                if (p <= nvalid) { PH[p] = (i >= 0) ? fm_phase(xv[u].y, xv[u].x) : prev; }  // (i == -1: the discriminator's previous phase; further back: not used)
            }
        }
        wave_sync();
        // d[s] over PH[s], a chunk of 64 at a time (lane l reads what lane l + 1 overwrites: both operands first, then the store); in front of the block: the line
        for (int s0 = 0; s0 < nvalid; s0 += 64) {
            const int s = s0 + lane, i = base + s;
            float d = 0.0f;
            if (s < nvalid) {
                d = normalize_phase(PH[s + 1] - PH[s]) * job.inv_deviation;
                if (i < 0) { d = global_load_f32(line, (K - 1) + i); }  // (i >= -(K - 1))
            }
            wave_sync();
            if (s < nvalid) { PH[s] = d; }
        }
        wave_sync();
        float acc[4] = { 0.0f, 0.0f, 0.0f, 0.0f };
        const float* w = PH + lane;
        for (int k = 0; k < K; k++) {
            const float h = taps[k];
#pragma unroll
            for (int r = 0; r < 4; r++) { acc[r] = acc[r] + (w[64 * r + k] * h); }  // (lanes past the tile's end read what an earlier tile left there: finite or not, never stored)
        }
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int j = lane + 64 * r;
            if (j < cnt && dst0 + j >= 0) { global_store_f32_boff(dst, (unsigned)(dst0 + j) * 4u, acc[r]); }
        }
        // the tail tile's window ends with the block's newest K - 1 values of d (the old line's where the block is shorter), behind them the last sample's phase
        if (tail && lane < K) { global_store_f32_boff(line_new, (unsigned)lane * 4u, PH[nvalid - (K - 1) + lane]); }
        wave_sync();  // (the next tile overwrites the window)
    }
}

// ---- loop: MM's recursion -----------------------------------------------------------------------------------------------------------------
// A LANE per VFO; lane v walks the symbols of its own stream.  Per symbol the reference's float operations in its order (the library is built without
// contraction): phase index, the T-tap dot product k-ascending (product and sum rounded apart), error, clamp, pcl.advance, floorf, offset and phase.
// LAYOUT: nothing is staged.  A symbol at `offset` reads the T floats buf[offset .. offset + T) of its lane's own row and the T floats of one bank phase,
// both straight from global memory, in one wait.  The bank (128 x 8 floats: 4 KB, one per context) does not fit a wavefront's share of the role's LDS beside
// rows of 64 VFOs, so its read is a cached load on the symbol's dependency chain in any layout; rows staged through LDS would take 64 x (chunk + T - 1)
// floats of the stride (chunks of 5 samples at T = 8: less than a symbol) and a second pass over every sample.  The kind uses no LDS at all and leaves the
// role's occupancy what it is; with T = 8 (the reference's only interpolator) row and phase are four 16-byte loads per symbol.
// COST (MI355X, profiles/pager_rate.md): at most 1.8 .. 1.9 us per symbol and wavefront of 64 lanes — an upper bound: the time of the branch's two launches
// per block (front and loop) divided by the symbols a lane walks; the loop's own share was not separated — and 3.5 us where two loop jobs share a workgroup.
// About 4 000 clocks, and it is the ROW's read they wait for, not the bank's: the bank stays in L1, the row was written by another CU and is asked for only
// when its symbol needs it.  64 channels still run at 220 x real time.  FOLLOW-UP, neither measured yet: (1) the next symbol's row requested a step ahead —
// its offset is known to +- ceil(|mu gain|) once the phase is, T + 2 floats cover it; (2) packs of 8 or 16 VFOs with rows staged through LDS, the next
// chunk's loads in flight as in the stereo loop (a chunk then holds several symbols); and a loop job per workgroup in either.
// Outputs: soft values and their slices (soft > 0.0f) by vector stores, symbol by symbol; the per-push symbol counts of a launch group at every push end.
struct SymLoopVfo {
    const float* buf;     // the front's [T - 1][n]
    float* soft;          // the block's symbols, all pushes of a launch group in one piece
    uint8_t* bits;
    int* counts;          // symbols per push
    float* state;         // pcl.phase, pcl.freq, lastOut, offset (an int's bits): persistent (device)
    const float* bank;    // phases x T, phase-major
    const int* ends;      // a launch group: the cumulative push ends at this stream's rate (nullptr: one push, n)
    float alpha, beta, min_freq, max_freq;  // mu gain, omega gain, omega limits
    int phases, T;
    int n, npush;
    int cap;              // symbols soft / bits have room for (never reached by a description sym_apply has taken: a bound on the stores all the same)
    int pad;
};
struct SymLoopJob {
    const SymLoopVfo* vfos;
    int nv, pad;
};
static_assert(SDRPP_SYM_PACK >= 1 && SDRPP_SYM_PACK <= 64, "a lane per VFO");
static_assert(sizeof(SymLoopVfo) % 8 == 0, "records lie in an array");
__device__ __forceinline__ float sym_step(float x) { return (x > 0.0f) ? 1.0f : -1.0f; }  // math/step.h
__device__ __forceinline__ void vfo_sym_loop_body(const SymLoopVfo* __restrict__ vfos, int nv) {
    const int lane = threadIdx.x & 63;
    if (lane >= nv) { return; }
    const SymLoopVfo me = vfos[lane];
    float phase = global_load_f32(me.state, 0), freq = global_load_f32(me.state, 1), last = global_load_f32(me.state, 2);
    int off = __float_as_int(global_load_f32(me.state, 3));
    const int T = me.T;
    const float fphases = (float)me.phases;
    int nsym = 0;
    for (int q = 0; q < me.npush; q++) {
        const int end = me.ends ? global_load_i32(me.ends, q) : me.n;
        int cnt = 0;
        while (off < end && nsym < me.cap) {
            int p = (int)floorf(phase * fphases);
            p = min(max(p, 0), me.phases - 1);
            float out = 0.0f;
            if (T == 8) {
                const float4 x0 = global_load_f32x4_unaligned(me.buf, off), x1 = global_load_f32x4_unaligned(me.buf, off + 4);
                const float4 h0 = global_load_f32x4(reinterpret_cast<const float4*>(me.bank), 2 * p), h1 = global_load_f32x4(reinterpret_cast<const float4*>(me.bank), 2 * p + 1);
                out = out + (x0.x * h0.x);
                out = out + (x0.y * h0.y);
                out = out + (x0.z * h0.z);
                out = out + (x0.w * h0.w);
                out = out + (x1.x * h1.x);
                out = out + (x1.y * h1.y);
                out = out + (x1.z * h1.z);
                out = out + (x1.w * h1.w);
            }
            else {
                for (int k = 0; k < T; k++) { out = out + (global_load_f32(me.buf, off + k) * global_load_f32(me.bank, p * T + k)); }
            }
            global_store_f32_boff(me.soft, (unsigned)nsym * 4u, out);
            me.bits[nsym] = (out > 0.0f) ? (uint8_t)1 : (uint8_t)0;
            nsym++;
            cnt++;
            float error = (sym_step(last) * out) - (last * sym_step(out));
            last = out;
            if (error > 1.0f) { error = 1.0f; }
            if (error < -1.0f) { error = -1.0f; }
            freq = freq + (me.beta * error);
            if (freq > me.max_freq) { freq = me.max_freq; }
            else if (freq < me.min_freq) { freq = me.min_freq; }
            phase = phase + (freq + (me.alpha * error));
            const float delta = floorf(phase);
            // (offset += delta: an int plus a float, exact below 2^24; a description sym_apply has taken steps 1 .. SDRPP_SYM_MAX_STEP + 1 samples — the bounds
            // only keep samples that are not numbers from carrying the walk out of the block)
            int step = (int)delta;
            step = (step >= 1) ? step : 1;
            step = (step <= SDRPP_SYM_MAX_STEP + 2) ? step : SDRPP_SYM_MAX_STEP + 2;
            off += step;
            phase = phase - delta;
        }
        global_store_u32(me.counts, q, (unsigned)cnt);
    }
    off = ((off > me.n) ? off : me.n) - me.n;
    global_store_f32_boff(me.state, 0u, phase);
    global_store_f32_boff(me.state, 4u, freq);
    global_store_f32_boff(me.state, 8u, last);
    global_store_f32_boff(me.state, 12u, __int_as_float(off));
}

// (calls, not inlined, as the stereo branch's bodies are: the role's own code and the tick kernel's register allocation stay what they are; the records are read
// with scalar loads, wave_uniform_job)
__device__ __attribute__((noinline)) void vfo_sym_front_call(const SymFrontJob* j, float* smem) { vfo_sym_front_body(wave_uniform_job(j), smem); }
__device__ __attribute__((noinline)) void vfo_sym_loop_call(const SymLoopJob* j) {
    const SymLoopJob job = wave_uniform_job(j);
    vfo_sym_loop_body(job.vfos, min(job.nv, SDRPP_SYM_PACK));
}

}  // namespace sdrpp_k
