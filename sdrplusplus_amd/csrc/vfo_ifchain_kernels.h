// The radio's IF chain: noise blanker and power squelch; FMIF (vfo_fmif_kernels.h), the RDS branch's jobs (vfo_rds_kernels.h) and the stereo branch's
// (vfo_stereo_kernels.h) run under the same job record.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <sdrpp_gfx950.h>
#include "vfo_fmif_kernels.h"
#include "vfo_rds_kernels.h"
#include "vfo_stereo_kernels.h"

namespace sdrpp_k {

// =====================================================================================================================
// The radio's IF chain between the RxVFO and the demodulator (radio_module.h:84-96): NoiseBlanker -> PowerSquelch on the complex IF.
//   NoiseBlanker (noise_reduction/noise_blanker.h:38-57), per sample, state `amp`:
//       inAmp = |x|;  if inAmp != 0: amp = amp * (1 - rate) + inAmp * rate;  excess = inAmp / amp;  if excess > level: x /= excess
//   PowerSquelch (noise_reduction/power_squelch.h:33-50), per reference BLOCK of the blanker's output: mean |x| in dB against the level,
//       the block is passed or zeroed.
// One WAVEFRONT per VFO, as in vfo_sequential_body: a coalesced load of 64 samples, |x| and |x| * rate for all of them at once, only the
// tracker's multiply + add left in the uniform loop (same operations in the same order as the reference: bit-identical state whatever the
// chunking), then excess, compare and gain as one parallel step.  The squelch's sum is a lane-partial sum reduced per block (positive terms:
// at most count * 2^-24 relative from the reference's sequential sum, 4e-4 dB for the reference's largest block); a closed block is written
// and then zero-filled by the same lanes.
// =====================================================================================================================
__device__ __forceinline__ void vfo_ifchain_body(int id, const IfcJob* __restrict__ jobs, float* smem) {
    const IfcJob job = jobs[id];
    if (job.kind == 1) {
        vfo_fmif_body(job, smem);
        return;
    }
    if (job.kind >= 5) {  // the WFM demodulator's stereo branch (vfo_stereo_kernels.h): `in` names the job's own record(s)
        if (job.kind == 5) { vfo_stereo_pilot_call(reinterpret_cast<const StereoPilotJob*>(job.in), smem); }
        else if (job.kind == 6) { vfo_stereo_loop_call(reinterpret_cast<const StereoLoopJob*>(job.in), smem); }
        else { vfo_stereo_matrix_call(reinterpret_cast<const StereoMatrixJob*>(job.in), smem); }
        return;
    }
    if (job.kind >= 2) {  // the WFM demodulator's RDS branch (vfo_rds_kernels.h): `in` names the job's own record
        if (job.kind == 2) { vfo_rds_front_call(reinterpret_cast<const RdsJob*>(job.in), smem); }
        else if (job.kind == 4) { vfo_rds_line_call(reinterpret_cast<const RdsLineJob*>(job.in)); }
        else { vfo_rds_rotate_exact_call(reinterpret_cast<const RdsRotXJob*>(job.in)); }
        return;
    }
    const int lane = threadIdx.x & 63;
    const int nblk = job.bounds ? job.nb : 1;
    float amp = job.nb_on ? *job.amp : 1.0f;
    int blk_lo = 0;
    for (int blk = 0; blk < nblk; blk++) {
        const int n = job.bounds ? job.bounds[blk] : job.n;  // end of this reference block
        float part = 0.0f;
        if (!job.nb_on) {
            // squelch alone: nothing sequential — four chunks' loads in flight per round (a chunk at a time the walk is one memory round trip per 64 samples)
            constexpr int U = 4;
            for (int base = blk_lo; base < n; base += 64 * U) {
                float2 xv[U];
#pragma unroll
                for (int u = 0; u < U; u++) {
                    const int i = base + 64 * u + lane;
                    xv[u] = (i < n) ? job.in[i] : make_float2(0.0f, 0.0f);
                }
#pragma unroll
                for (int u = 0; u < U; u++) {
                    const int i = base + 64 * u + lane;
                    if (i < n) {
                        part += sqrtf((xv[u].x * xv[u].x) + (xv[u].y * xv[u].y));  // (chunk after chunk per lane: the same partial sums as a one-chunk walk)
                        job.out[i] = xv[u];
                    }
                }
            }
        }
        else {
            float2 xnext = (blk_lo + lane < n) ? job.in[blk_lo + lane] : make_float2(0.0f, 0.0f);
            for (int base = blk_lo; base < n; base += 64) {
                const int cnt = (n - base < 64) ? n - base : 64;
                float2 x = xnext;
                if (base + 64 + lane < n) { xnext = job.in[base + 64 + lane]; }  // the next chunk travels while the tracker walks this one
                const float a_l = sqrtf((x.x * x.x) + (x.y * x.y));
                const float t_l = a_l * job.nb_rate;
                float my_amp = 1.0f;
                for (int i = 0; i < cnt; i++) {
                    const float na = (amp * job.nb_inv_rate) + wave_bcast(t_l, i);
                    amp = (wave_bcast(a_l, i) != 0.0f) ? na : amp;  // (a select, not a branch: the chain is multiply, add, select)
                    if (lane == i) { my_amp = amp; }
                }
                if (a_l != 0.0f) {
                    const float excess = a_l / my_amp;
                    if (excess > job.nb_level) {
                        const float gain = 1.0f / excess;
                        x.x = x.x * gain;
                        x.y = x.y * gain;
                    }
                }
                if (lane < cnt) {
                    if (job.sq_on) { part += sqrtf((x.x * x.x) + (x.y * x.y)); }
                    job.out[base + lane] = x;
                }
            }
        }
        if (job.sq_on && n > blk_lo) {
            float sum = wave_sum(part);
            sum /= (float)(n - blk_lo);
            if (!(10.0f * log10f(sum) >= job.sq_level)) {
                for (int i = blk_lo + lane; i < n; i += 64) { job.out[i] = make_float2(0.0f, 0.0f); }  // (lane l rewrites what lane l wrote)
            }
        }
        if (n > blk_lo) { blk_lo = n; }
    }
    if (job.nb_on && lane == 0) { *job.amp = amp; }
}
// four jobs per workgroup, one per wavefront (gx = ceil(njobs / 4)): the shape the role has inside a tick.  LDS: 4 * SDRPP_FMIF_LDS_WAVE floats where
// the table holds FMIF segments, none otherwise.
__global__ __launch_bounds__(256) void vfo_ifchain_kernel(const IfcJob* __restrict__ jobs, int njobs) {
    HIP_DYNAMIC_SHARED(float, smemi)
    const int j = (int)blockIdx.x * 4 + ((int)threadIdx.x >> 6);
    if (j < njobs) { vfo_ifchain_body(j, jobs, smemi); }
}

}  // namespace sdrpp_k
