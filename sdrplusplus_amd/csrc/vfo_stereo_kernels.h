// The WFM demodulator's stereo branch: pilot filter, pilot PLL, L-R matrix and the L / R audio low-passes.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <sdrpp_gfx950.h>
#include "vfo_fir_kernels.h"
#include "vfo_math.h"
#include "vfo_stream.h"

namespace sdrpp_k {

// =====================================================================================================================
// BroadcastFM's _stereo path (demod/broadcast_fm.h:147-191), per IF sample i:
//     m[i]  = Quadrature(x[i])                                   (quadrature.h:39-46; fm_phase / normalize_phase, as the audio low-pass takes it)
//     p[i]  = sum_k (m[i - (K-1) + k] + 0j) * h[k]               (FIR<complex_t, complex_t>, K complex taps of taps::bandPass<complex_t>)
//     v[i]  = phasor(phase);  advance(normalizePhase(arg p[i] - phase))      (loop::PLL, pll.h:64-70; phase_control_loop.h:58-85)
//     q     = (m[i - D] + 0j) * conj(v[i]) * conj(v[i]);  lmr = 2 q.re;  l = m[i - D] + lmr,  r = m[i - D] - lmr;  alFir(l), arFir(r)
// Three kinds of the wavefront-job role (vfo_ifchain_kernels.h), a level each:
//   pilot   (WK_ST_PILOT) everything in front of the loop: parallel over samples, a wavefront per run of SDRPP_ST_SEG samples
//   loop    (WK_ST_LOOP) the recursion alone: a LANE per VFO, up to SDRPP_ST_PACK VFOs per wavefront (StereoLoopJob: a run of StereoLoopVfo records)
//   matrix  (WK_ST_MATRIX) everything behind the loop: parallel over samples, a wavefront per run of SDRPP_ST_SEG samples
// Every sum is a k-ascending fmaf chain per output and every job boundary a function of the block alone: results do not depend on the cut.
// Each wavefront works in its share of the role's LDS (SDRPP_WAVE_LDS_FLOATS floats: jobs of every kind share a workgroup).
// =====================================================================================================================
#ifndef SDRPP_WAVE_LDS_FLOATS
#error "a part of vfo_ifchain_kernels.h, the role's header: include that one"
#endif
#define SDRPP_ST_SEG 1024          // samples per pilot / matrix job
#define SDRPP_ST_PILOT_TILE 256    // pilot: outputs per tile (four per lane); its window of tile + K values must fit: K <= SDRPP_ST_PILOT_MAX_TAPS
#define SDRPP_ST_MATRIX_TILE 128   // matrix: frames per tile (two per lane); two windows of tile + K - 1 values: K <= SDRPP_ST_AUDIO_MAX_TAPS
#define SDRPP_ST_PILOT_MAX_TAPS (SDRPP_WAVE_LDS_FLOATS - SDRPP_ST_PILOT_TILE)
#define SDRPP_ST_AUDIO_MAX_TAPS (SDRPP_WAVE_LDS_FLOATS / 2 - SDRPP_ST_MATRIX_TILE + 1)
#define SDRPP_ST_PACK 8            // loop: VFOs per wavefront (the fewer, the longer the chunks a wavefront stages and the more wavefronts share the work)
#define SDRPP_ST_LOOP_CHUNK 256    // loop: elements of all rows together a wavefront stages per chunk (four per lane: what it holds in registers while the previous chunk is walked)
#define SDRPP_ST_LOOP_PTRS 64      // loop: floats of the wavefront's LDS in front of the rows: per row its two addresses and its length (StereoLoopRow)

// ---- pilot: discriminator -> complex band-pass on the real stream -> phase angle ---------------------------------------------------------
// One pass over the IF stream per tile: the phases of the tile's samples and of the K samples in front of them (the stream's history included)
// are taken ONCE into LDS and become their differences in place (the window of m); lane j then accumulates outputs j, j + 64, j + 128, j + 192
// of the tile — consecutive lanes read consecutive addresses, taps are wave-uniform scalar loads.
struct StereoPilotJob {
    StreamIn in;        // the stream the demodulator reads (complex); its history holds at least K samples
    float* m;           // discriminator values of this block
    float* ang;         // atan2(p.im, p.re) of this block
    const float* taps;  // K complex taps, interleaved, natural order
    int K;
    int lo, hi;         // the samples of this job
    float inv_deviation;
};
__device__ __forceinline__ void vfo_stereo_pilot_body(const StereoPilotJob& job, float* smem) {
    const int lane = threadIdx.x & 63, wv = (int)threadIdx.x >> 6;
    const int K = job.K;
    float* PH = smem + wv * SDRPP_WAVE_LDS_FLOATS;  // phases, then (in place) the window of m
    const UniformF32 taps = as_uniform(job.taps);
    for (int t0 = job.lo; t0 < job.hi; t0 += SDRPP_ST_PILOT_TILE) {
        const int cnt = min(SDRPP_ST_PILOT_TILE, job.hi - t0);
        const int base = t0 - (K - 1);     // stream index of window element 0
        const int nvalid = cnt + K - 1;    // window elements; PH[p] = phase of stream sample base - 1 + p, p = 0 .. nvalid
        constexpr int U = 4;
        for (int p0 = lane; p0 <= nvalid; p0 += 64 * U) {
            float2 xv[U];
#pragma unroll
            for (int u = 0; u < U; u++) {
                const int p = p0 + 64 * u, i = base - 1 + p;
                xv[u] = stream_load2_nb(job.in, i, p <= nvalid && i >= -job.in.hist_len);
            }
#pragma unroll
            for (int u = 0; u < U; u++) {
                const int p = p0 + 64 * u;
                if (p <= nvalid) { PH[p] = fm_phase(xv[u].y, xv[u].x); }
            }
        }
        wave_sync();
        // m[s] over PH[s], a chunk of 64 at a time (lane l reads what lane l + 1 overwrites: both operands first, then the store)
        for (int s0 = 0; s0 < nvalid; s0 += 64) {
            const int s = s0 + lane;
            float d = 0.0f;
            if (s < nvalid) { d = normalize_phase(PH[s + 1] - PH[s]) * job.inv_deviation; }
            wave_sync();
            if (s < nvalid) { PH[s] = d; }
        }
        wave_sync();
        float re[4] = { 0.0f, 0.0f, 0.0f, 0.0f }, im[4] = { 0.0f, 0.0f, 0.0f, 0.0f };
        const float* w = PH + lane;
        for (int k = 0; k < K; k++) {
            const float tr = taps[2 * k], ti = taps[2 * k + 1];
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const float x = w[64 * r + k];  // (lanes past the tile's end read what the previous tile left there: finite or not, never stored)
                re[r] = fmaf(x, tr, re[r]);
                im[r] = fmaf(x, ti, im[r]);
            }
        }
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int j = lane + 64 * r;
            if (j < cnt) {
                global_store_f32_boff(job.m, (unsigned)(t0 + j) * 4u, PH[j + K - 1]);
                global_store_f32_boff(job.ang, (unsigned)(t0 + j) * 4u, fm_phase(im[r], re[r]));
            }
        }
        wave_sync();  // (the next tile overwrites the window)
    }
}

// ---- loop: the PLL's recursion ---------------------------------------------------------------------------------------------------------
// Nothing but the recursion is left here: subtract, normalise, two multiply-adds, clamp, wrap — the reference's float operations in its order
// (the library is built without contraction).  A LANE per VFO: the wavefront stages a chunk of every VFO's angles through LDS — loads and stores
// run over the rows' elements in order, consecutive lanes on consecutive addresses of a row — and lane v walks row v; rows lie `pitch` floats apart,
// an odd number, so the lanes' accesses of one step fall on different banks.  While a chunk is walked the next one's loads are in flight.
// The phase the loop had BEFORE each update is written back in place and stored as the sample's loop phase.
struct StereoLoopVfo {
    const float* ang;  // the pilot job's angles of this block
    float* ph;         // the loop phase per sample
    float2* state;     // (phase, freq), persistent (device)
    float alpha, beta, min_freq, max_freq;
    int n;
};
struct StereoLoopRow { const float* ang; float* ph; int n, pad; };
// One loop job: `nv` consecutive records, staged `chunk` samples of every row at a time into rows `pitch` floats apart (the planner: chunk =
// SDRPP_ST_LOOP_CHUNK / nv, pitch = chunk | 1); nmax: the longest row
struct StereoLoopJob {
    const StereoLoopVfo* vfos;
    int nv, chunk, pitch, nmax;
};
static_assert(SDRPP_ST_PACK >= 1 && SDRPP_ST_PACK <= 64, "a lane per VFO");
static_assert(SDRPP_ST_PACK * sizeof(StereoLoopRow) <= SDRPP_ST_LOOP_PTRS * sizeof(float), "the rows' descriptions fit in front of the rows");
static_assert(SDRPP_ST_LOOP_CHUNK % 64 == 0 && SDRPP_ST_LOOP_CHUNK < 65536, "whole elements per lane; a column fits 16 bits");
// (nv rows of pitch = (CHUNK / nv) | 1 <= CHUNK / nv + 1 floats: at most CHUNK + nv floats)
static_assert(SDRPP_ST_LOOP_PTRS + SDRPP_ST_LOOP_CHUNK + SDRPP_ST_PACK <= SDRPP_WAVE_LDS_FLOATS, "the rows of a chunk fit the wavefront's share of the role's LDS");
__device__ __forceinline__ void vfo_stereo_loop_body(const StereoLoopVfo* __restrict__ vfos, int nv, int C, int pitch, int nmax, float* smem) {
    const int lane = threadIdx.x & 63, wv = (int)threadIdx.x >> 6;
    StereoLoopRow* AD = reinterpret_cast<StereoLoopRow*>(smem + wv * SDRPP_WAVE_LDS_FLOATS);  // nv <= SDRPP_ST_PACK rows
    float* ROW = smem + wv * SDRPP_WAVE_LDS_FLOATS + SDRPP_ST_LOOP_PTRS;
    const float FL_PI = 3.1415926535f, TWO_PI = FL_PI - (-FL_PI);  // phase_control_loop.h:28: phaseDelta = maxPhase - minPhase
    const bool mine = lane < nv;
    const StereoLoopVfo me = vfos[mine ? lane : 0];
    float phase = 0.0f, freq = 0.0f;
    if (mine) {
        const float2 s = global_load_f32x2(me.state, 0);
        phase = s.x;
        freq = s.y;
        AD[lane] = StereoLoopRow{ me.ang, me.ph, me.n, 0 };
    }
    const int n_mine = mine ? me.n : 0;
    wave_sync();
    constexpr int Q = SDRPP_ST_LOOP_CHUNK / 64;  // elements per lane of a chunk
    const int total = nv * C;
    // element e of a chunk: row e / C, column e % C
    // (row << 16 | column per element and nothing else kept in registers: the rows' addresses and lengths are read back from LDS; -1: no element)
    int erc[Q];
#pragma unroll
    for (int q = 0; q < Q; q++) {
        const int e = lane + 64 * q, r = e / C;
        erc[q] = (e < total) ? ((r << 16) | (e - r * C)) : -1;
    }
    float pf[Q];
    auto fetch = [&](int c0) {
#pragma unroll
        for (int q = 0; q < Q; q++) {
            const StereoLoopRow& row = AD[erc[q] >= 0 ? erc[q] >> 16 : 0];
            const int i = c0 + (erc[q] & 0xffff);
            pf[q] = global_load_f32(row.ang, (erc[q] >= 0 && i < row.n) ? i : 0);  // (element 0 of a row's buffer always exists)
        }
    };
    if (nmax > 0) { fetch(0); }
    for (int c0 = 0; c0 < nmax; c0 += C) {
#pragma unroll
        for (int q = 0; q < Q; q++) {
            if (erc[q] >= 0) { ROW[(erc[q] >> 16) * pitch + (erc[q] & 0xffff)] = pf[q]; }
        }
        wave_sync();
        if (c0 + C < nmax) { fetch(c0 + C); }
        float* row = ROW + lane * pitch;
        const int cnt = min(C, n_mine - c0);
        for (int j = 0; j < cnt; j++) {
            const float a = row[j];
            row[j] = phase;
            const float err = normalize_phase(a - phase);
            freq = freq + (me.beta * err);
            if (freq > me.max_freq) { freq = me.max_freq; }
            else if (freq < me.min_freq) { freq = me.min_freq; }
            phase = phase + (freq + (me.alpha * err));
            while (phase > FL_PI) { phase -= TWO_PI; }
            while (phase < -FL_PI) { phase += TWO_PI; }
        }
        wave_sync();
#pragma unroll
        for (int q = 0; q < Q; q++) {
            if (erc[q] >= 0) {
                const StereoLoopRow& row = AD[erc[q] >> 16];
                const int i = c0 + (erc[q] & 0xffff);
                if (i < row.n) { global_store_f32_boff(row.ph, (unsigned)i * 4u, ROW[(erc[q] >> 16) * pitch + (erc[q] & 0xffff)]); }
            }
        }
        wave_sync();  // (the next chunk overwrites the rows)
    }
    if (mine) { global_store_f32x2(me.state, 0, make_float2(phase, freq)); }
}

// ---- matrix: phasor of the stored loop phase, the two complex products, l and r, the two audio low-passes ----------------------------------
// Per tile the wavefront forms l and r in front of the filters for the tile's frames and the K - 1 in front of them in LDS — from m[i - D] and the
// stored loop phases, histories included: what the reference keeps in two delay lines and two filter lines is recomputed, bit for bit, from the two
// streams' histories — and lane j accumulates frames j and j + 64 of both channels.  K = 1 (a unit tap) is the reference with its low-pass off.
struct StereoMatrixJob {
    StreamIn m;         // discriminator values (real); history of at least D + K - 1
    StreamIn ph;        // loop phases (real); history of at least K - 1
    float2* out;        // (l, r) frames
    const float* taps;  // K audio taps, natural order
    int K, D;
    int lo, hi;
};
__device__ __forceinline__ void vfo_stereo_matrix_body(const StereoMatrixJob& job, float* smem) {
    const int lane = threadIdx.x & 63, wv = (int)threadIdx.x >> 6;
    const int K = job.K;
    constexpr int P = SDRPP_WAVE_LDS_FLOATS / 2;
    float* LW = smem + wv * SDRPP_WAVE_LDS_FLOATS;
    float* RW = LW + P;
    const UniformF32 taps = as_uniform(job.taps);
    for (int t0 = job.lo; t0 < job.hi; t0 += SDRPP_ST_MATRIX_TILE) {
        const int cnt = min(SDRPP_ST_MATRIX_TILE, job.hi - t0);
        const int base = t0 - (K - 1), nvalid = cnt + K - 1;
        constexpr int U = 2;
        for (int p0 = lane; p0 < nvalid; p0 += 64 * U) {
            float md[U], th[U];
#pragma unroll
            for (int u = 0; u < U; u++) {
                const int p = p0 + 64 * u, i = base + p;
                md[u] = stream_load1_nb(job.m, i - job.D, p < nvalid && i - job.D >= -job.m.hist_len);
                th[u] = stream_load1_nb(job.ph, i, p < nvalid && i >= -job.ph.hist_len);
            }
#pragma unroll
            for (int u = 0; u < U; u++) {
                const int p = p0 + 64 * u;
                if (p < nvalid) {
                    LW[p] = md[u];
                    RW[p] = th[u];
                }
            }
        }
        // (one sample per lane at a time, each lane on the elements it wrote itself: a single instance of the phasor keeps the body's registers few)
#pragma unroll 1
        for (int p = lane; p < nvalid; p += 64) {
            const float md = LW[p], th = fminf(fmaxf(RW[p], -4.0f), 4.0f);  // (the loop wraps its phase to +-pi: the bound only tells the compiler that no large-argument reduction is needed)
            // (md + 0j) * conj(v) * conj(v), v = (cosf, sinf): every product of the reference's complex multiply in place, rounded on its own
            const float vr = cosf(th), vi = -sinf(th);
            const float ar = (md * vr) - (0.0f * vi), ai = (md * vi) + (0.0f * vr);
            const float qr = (ar * vr) - (ai * vi);
            const float lmr = qr * 2.0f;
            LW[p] = md + lmr;
            RW[p] = md - lmr;
        }
        wave_sync();
        float al[2] = { 0.0f, 0.0f }, ar2[2] = { 0.0f, 0.0f };
        for (int k = 0; k < K; k++) {
            const float h = taps[k];
#pragma unroll
            for (int r = 0; r < 2; r++) {
                al[r] = fmaf(h, LW[lane + 64 * r + k], al[r]);
                ar2[r] = fmaf(h, RW[lane + 64 * r + k], ar2[r]);
            }
        }
#pragma unroll
        for (int r = 0; r < 2; r++) {
            const int j = lane + 64 * r;
            if (j < cnt) { global_store_f32x2(job.out, t0 + j, make_float2(al[r], ar2[r])); }
        }
        wave_sync();  // (the next tile overwrites the windows)
    }
}

// (calls, not inlined, as the RDS branch's bodies are: the role's own code and the tick kernel's register allocation stay what they are.  What a call is
// handed arrives in vector registers although every lane holds the same: the job's address is stated to be wave-uniform and its record read with scalar
// loads (wave_uniform_job), so that the record, and every address and bound computed from it, stays in scalar registers)
__device__ __attribute__((noinline)) void vfo_stereo_pilot_call(const StereoPilotJob* j, float* smem) { vfo_stereo_pilot_body(wave_uniform_job(j), smem); }
__device__ __attribute__((noinline)) void vfo_stereo_loop_call(const StereoLoopJob* j, float* smem) {
    const StereoLoopJob job = wave_uniform_job(j);
    vfo_stereo_loop_body(job.vfos, min(job.nv, SDRPP_ST_PACK), job.chunk, job.pitch, job.nmax, smem);
}
__device__ __attribute__((noinline)) void vfo_stereo_matrix_call(const StereoMatrixJob* j, float* smem) { vfo_stereo_matrix_body(wave_uniform_job(j), smem); }

}  // namespace sdrpp_k
