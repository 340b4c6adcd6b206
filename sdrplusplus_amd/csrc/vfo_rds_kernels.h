// The WFM demodulator's RDS branch: discriminator -> translation by -57 kHz -> first decimator, fused; and the same translation as the reference's float recursion.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <sdrpp_gfx950.h>
#include "vfo_fir_kernels.h"
#include "vfo_math.h"
#include "vfo_rot_kernels.h"
#include "vfo_stream.h"

namespace sdrpp_k {

// =====================================================================================================================
// BroadcastFM's _rdsOut path (demod/broadcast_fm.h:144-215) up to the first stage of its RationalResampler<complex_t>:
//     d[i] = normalizePhase(atan2f(x[i]) - atan2f(x[i-1])) * invDeviation        (quadrature.h:39-46; fm_phase / normalize_phase, as the audio low-pass takes it)
//     c[i] = (d[i] + 0j) * e^{j 2 pi (phi + (i - anchor) * theta)}               (FrequencyXlator(-57 kHz), closed form: float64 turns, anchored per push)
//     y[m] = sum_k h[k] * c[off0 + m * D - (K-1) + k]                            (PowerDecimator's first DecimatingFIR, D : 1, K real taps on the complex stream)
// in ONE pass over the IF stream: neither d nor c ever goes to memory.  One WAVEFRONT per job (a run of outputs of one push, walked a tile of
// `tile` outputs at a time) under the wavefront-job role, four jobs per workgroup, SDRPP_WAVE_LDS_FLOATS floats of LDS each (the role's stride):
//   1. the tile's (tile - 1) * D + K IF samples and the one in front of them — the stream's history in front of the block included — are fetched
//      four loads in flight per lane, their phases taken ONCE per sample into LDS;
//   2. the phases become their differences in place, and c = d * phasor goes into the window, de-interleaved by decimation phase: sample s at
//      [s mod D][s div D], rows `pitch` float2 apart.  The pitch is chosen by the host (rds_tile_geometry) so that the 16 lanes an 8-byte store is
//      carried out for at a time, which hold 16 consecutive samples, meet 16 different 8-byte banks (D = 8: pitch = 2 mod 4);
//   3. lane j accumulates output j of the tile: tap k multiplies [k mod D][j + k div D] — consecutive lanes, consecutive addresses, no bank
//      conflict; taps are wave-uniform scalar loads.  The sum is the k-ascending fmaf chain of the project's other FIRs, whatever tile or cut.
// The first decimator's delay line holds discriminator VALUES.  Normally they are recomputed from the stream's history (job.in.hist).  After the branch
// was attached, switched off, reset around or moved, the stream's history is not what the branch has seen: the values are then taken from the line that
// was set aside (job.dline: the K newest d the branch was fed, newest last; vfo_rds_line_body keeps it up while blocks shorter than the line arrive),
// and nothing in front of the block is read.  d[0] always belongs to the running discriminator: job.prev0, the stream's true last sample.
// =====================================================================================================================
#ifndef SDRPP_WAVE_LDS_FLOATS
#error "a part of vfo_ifchain_kernels.h, the role's header: include that one"
#endif
struct RdsJob {
    StreamIn in;          // the stream the demodulator reads: this block's samples, and the history the branch's delay line is recomputed from
    const float2* prev0;  // the sample in front of in.data[0] as the discriminator sees it
    float2* out;
    const float* taps;    // K taps, natural order
    const float* dline;   // nullptr: d[i < 0] from in.hist; else the set-aside line, d[i] = dline[K + i] for i in -K .. -1 (in.hist_len is 0 then)
    int K, lgD;
    int off0;             // stream index of the newest sample under output 0's window
    int m_lo, m_hi;       // the outputs of this job
    int tile, pitch;      // outputs per tile (<= 64), float2 per decimation-phase row
    int anchor;           // stream index at which the NCO phase is `phi` (the first sample of the job's push)
    float inv_deviation;
    double theta, phi;    // turns per sample, turns
};

__device__ __forceinline__ void vfo_rds_front_body(const RdsJob& job, float* smem) {
    const int lane = threadIdx.x & 63, wv = (int)threadIdx.x >> 6;
    const int K = job.K, lgD = job.lgD, D = 1 << lgD, P = job.pitch;
    float2* C = reinterpret_cast<float2*>(smem + wv * SDRPP_WAVE_LDS_FLOATS);  // the window: D rows of P
    float* PH = smem + wv * SDRPP_WAVE_LDS_FLOATS + 2 * D * P;                 // phases, then (in place) their differences
    const UniformF32 taps = as_uniform(job.taps);
    const float2 x0 = global_load_f32x2(job.prev0, 0);
    for (int m0 = job.m_lo; m0 < job.m_hi; m0 += job.tile) {
        const int cnt = min(job.tile, job.m_hi - m0);
        const int base = job.off0 + (m0 << lgD) - (K - 1);  // stream index of window element 0
        const int nvalid = ((cnt - 1) << lgD) + K;
        // PH[p] = phase of stream sample base - 1 + p, p = 0 .. nvalid: four loads in flight per lane, none behind a branch
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
        // d[s] over PH[s], a chunk of 64 at a time (lane l reads what lane l + 1 overwrites: both operands first, then the store)
        for (int s0 = 0; s0 < nvalid; s0 += 64) {
            const int s = s0 + lane;
            float d = 0.0f;
            if (s < nvalid) {
                const int i = base + s;
                const float before = (i == 0) ? fm_phase(x0.y, x0.x) : PH[s];
                d = normalize_phase(PH[s + 1] - before) * job.inv_deviation;
                if (job.dline && i < 0) { d = global_load_f32(job.dline, K + i); }  // (i >= -(K - 1): the window's oldest element)
            }
            wave_sync();
            if (s < nvalid) { PH[s] = d; }
        }
        // c = d * phasor into the window (lane l reads back what it wrote itself)
        for (int s = lane; s < nvalid; s += 64) {
            float sn, cs;
            turn_sincos(fma((double)(base + s - job.anchor), job.theta, job.phi), sn, cs);
            const float d = PH[s];
            C[(s & (D - 1)) * P + (s >> lgD)] = make_float2(d * cs, d * sn);
        }
        wave_sync();
        if (lane < cnt) {
            float2 acc = make_float2(0.0f, 0.0f);
            const float2* cj = C + lane;
            for (int k = 0; k < K; k++) { cmac(taps[k], cj[(k & (D - 1)) * P + (k >> lgD)], acc); }
            global_store_f32x2(job.out, m0 + lane, acc);
        }
        wave_sync();  // (the next tile overwrites window and phases)
    }
}
// The set-aside line kept up: new_line = the K newest of (old_line ++ d(data[0 .. n))), d[0] against prev0.  One wavefront; n < K while short blocks are
// spliced on, n = K (old_line unused) when the line is taken from the stream's own history as the branch is switched off.
struct RdsLineJob {
    const float2* data;
    const float2* prev0;
    const float* old_line;
    float* new_line;
    int n, K;
    float inv_deviation;
};
__device__ __forceinline__ void vfo_rds_line_body(const RdsLineJob& job) {
    const int lane = threadIdx.x & 63;
    for (int e0 = 0; e0 < job.K; e0 += 64) {  // (every old value is read before any is written: old and new line may be the same buffer only for n >= K)
        const int e = e0 + lane, q = job.n + e - job.K;  // element e of the new line is element n + e of the sequence: old line, then this block's d[q]
        if (e < job.K) {
            float v;
            if (q < 0) { v = global_load_f32(job.old_line, job.n + e); }
            else {
                const float2 x = global_load_f32x2(job.data, q), xp = global_load_f32x2(q == 0 ? job.prev0 : job.data, q == 0 ? 0 : q - 1);
                v = normalize_phase(fm_phase(x.y, x.x) - fm_phase(xp.y, xp.x)) * job.inv_deviation;
            }
            job.new_line[e] = v;
        }
    }
}
__device__ __attribute__((noinline)) void vfo_rds_line_call(const RdsLineJob* j) { vfo_rds_line_body(*j); }
__global__ __launch_bounds__(64) void vfo_rds_line_kernel(RdsLineJob job) { vfo_rds_line_body(job); }

// (a call, not inlined, as the recorder's body is in the copy role: the role's own code and the tick kernel's register allocation stay what they are)
__device__ __attribute__((noinline)) void vfo_rds_front_call(const RdsJob* j, float* smem) { vfo_rds_front_body(*j, smem); }

// =====================================================================================================================
// The same translation as the reference runs it (frequency_xlator.h:43-50 around volk_32fc_s32fc_x2_rotator_32fc): the float recursion
// phase *= delta at the IF rate, renormalised every 512 samples and at the end of every reference block.  One WAVEFRONT per VFO after the
// pattern of vfo_ssb_rotate_exact_body: the lanes take the phases of a chunk of 64 samples and their differences at once, every lane walks
// the same (uniform) recursion and lane i keeps d[i] * phase of sample i.  The rotated stream goes to memory (a parity mode) and the first
// decimator then runs as a plain FIR over it.
// =====================================================================================================================
struct RdsRotXJob {
    const float2* in;     // this block's samples of the stream the demodulator reads
    const float2* prev0;  // the sample in front of them
    float2* out;          // d * phase, complex, at the IF rate
    float2* state;        // FrequencyXlator::phase, persistent (device)
    float dr, di;
    float inv_deviation;
    int n;
    const int* bounds;    // reference-block ends at the IF rate (nullptr: the block is one)
    int nb;
};
__device__ __forceinline__ void vfo_rds_rotate_exact_body(const RdsRotXJob& job) {
    const int lane = (int)threadIdx.x & 63;
    float pr = job.state->x, pi = job.state->y;
    const float2 x0 = global_load_f32x2(job.prev0, 0);
    float carry = fm_phase(x0.y, x0.x);  // phase of the sample in front of the chunk
    const int nblk = job.bounds ? job.nb : 1;
    int b0 = 0;
    for (int blk = 0; blk < nblk; blk++) {
        const int b1 = job.bounds ? job.bounds[blk] : job.n;
        int since = 0;
        for (int base = b0; base < b1; base += 64) {
            const int cnt = min(64, b1 - base);
            const float2 xv = (lane < cnt) ? global_load_f32x2(job.in, base + lane) : make_float2(0.0f, 0.0f);
            const float ph = fm_phase(xv.y, xv.x);
            const float d = normalize_phase(ph - wave_shr1(ph, carry)) * job.inv_deviation;
            carry = wave_bcast(ph, cnt - 1);
            float2 mine = make_float2(0.0f, 0.0f);
            for (int i = 0; i < cnt; i++) {
                const float di = wave_bcast(d, i);
                // (d + 0j) * phase with every product of the reference's complex multiply in place (rounded on its own: 0 * pi is +-0)
                const float re = (di * pr) - (0.0f * pi), im = (di * pi) + (0.0f * pr);
                if (lane == i) { mine = make_float2(re, im); }
                const float nr = (pr * job.dr) - (pi * job.di);
                const float ni = (pr * job.di) + (pi * job.dr);
                pr = nr;
                pi = ni;
                since++;
                if ((since & 511) == 0) { rotator_norm(pr, pi); }
            }
            if (lane < cnt) { global_store_f32x2(job.out, base + lane, mine); }
        }
        if ((since & 511) != 0) { rotator_norm(pr, pi); }
        if (b1 > b0) { b0 = b1; }
    }
    if (lane == 0) { *job.state = make_float2(pr, pi); }
}
__device__ __attribute__((noinline)) void vfo_rds_rotate_exact_call(const RdsRotXJob* j) { vfo_rds_rotate_exact_body(*j); }
// Front, line and rotator run as kinds of the wavefront-job role (WK_RDS_FRONT, WK_RDS_LINE, WK_RDS_ROTX, vfo_ifchain_kernels.h): in an ordinary pass
// vfo_ifchain_kernel is their launch, in a tick TR_IFC their role.

}  // namespace sdrpp_k
