// The tick's wavefront-job role (TR_IFC, `ifc`) and its stand-alone launch: one wavefront per job, four jobs per workgroup.  It began as the radio's IF
// chain (noise blanker / power squelch, below) and carries every piece of work that is one wavefront wide: FMIF (vfo_fmif_kernels.h), the RDS branch's jobs
// (vfo_rds_kernels.h), the stereo branch's (vfo_stereo_kernels.h), the symbol branch's (vfo_sym_kernels.h), the RDS demodulator (vfo_rdsd_kernels.h), the Meteor QPSK
// demodulator (vfo_qpsk_kernels.h) and the framer behind a symbol branch (vfo_frame_kernels.h).  Those seven headers are parts of this one.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <sdrpp_gfx950.h>

namespace sdrpp_k {

// What runs in a wavefront.  A new kind is a record struct, a `*_call` that reads it, an entry here, a case in vfo_wave_body and a file_wave line in the
// planner (BankPlan::upload).  The values never leave the library.
enum WaveKind : int { WK_NBSQ, WK_FMIF, WK_RDS_FRONT, WK_RDS_ROTX, WK_RDS_LINE, WK_ST_PILOT, WK_ST_LOOP, WK_ST_MATRIX, WK_SYM_FRONT, WK_SYM_LOOP, WK_RDS_DEMOD, WK_QPSK_FRONT, WK_QPSK_LOOP, WK_SYM_FRAME, WK_COUNT };
// The table the role reads: entry j is wavefront j's work.  `rec` is the kind's own record (NbSqJob, FmifJob, RdsJob, RdsRotXJob, RdsLineJob, StereoPilotJob,
// StereoLoopJob, StereoMatrixJob, SymFrontJob, SymLoopJob, RdsdJob, QpskFrontJob, QpskLoopJob, FrameJob); `arg` is the part of the record this wavefront takes where a record is cut into several jobs
// (FMIF and the QPSK front: the segment's first sample).
struct WaveJob {
    const void* rec;
    int kind;
    int arg;
};
static_assert(sizeof(WaveJob) == 16, "the role's table: 16 bytes per wavefront");
// the kinds that work in the wavefront's share of the role's LDS
constexpr bool wave_kind_uses_lds(int kind) { return kind == WK_FMIF || kind == WK_RDS_FRONT || kind == WK_ST_PILOT || kind == WK_ST_LOOP || kind == WK_ST_MATRIX || kind == WK_SYM_FRONT || kind == WK_RDS_DEMOD || kind == WK_QPSK_FRONT || kind == WK_QPSK_LOOP || kind == WK_SYM_FRAME; }  // (WK_SYM_LOOP reads its rows and its bank from global memory: vfo_sym_kernels.h)

// A record read by the whole wavefront: what a call is handed, and what a lane computes from its own index, lies in vector registers although every lane holds
// the same.  The address is stated to be wave-uniform and the record read with scalar loads, so that it, and every address and bound computed from it, stays in
// scalar registers.
template <class T>
__device__ __forceinline__ const T* wave_uniform_ptr(const T* p) {
    const uint64_t a = (uint64_t)(uintptr_t)p;
    const uint32_t lo = (uint32_t)wave_uniform((int)(uint32_t)a), hi = (uint32_t)wave_uniform((int)(uint32_t)(a >> 32));
    return reinterpret_cast<const T*>((uintptr_t)(((uint64_t)hi << 32) | (uint64_t)lo));
}
template <class T>
__device__ __forceinline__ T wave_uniform_job(const T* p) {
    static_assert(sizeof(T) % 4 == 0, "job records are whole words");
    const UniformI32 u = as_uniform_i32(wave_uniform_ptr(p));
    int w[sizeof(T) / 4];
#pragma unroll
    for (int i = 0; i < (int)(sizeof(T) / 4); i++) { w[i] = u[i]; }
    T job;
    __builtin_memcpy(&job, w, sizeof(T));
    return job;
}

}  // namespace sdrpp_k

// Floats of LDS per wavefront of the role: ONE stride, because jobs of every kind share a workgroup.  FMIF's window and exchange set it (the macros are
// vfo_fmif_kernels.h's); what every other kind needs is checked against it below.
#define SDRPP_WAVE_LDS_FLOATS ((SDRPP_FMIF_SEG + SDRPP_FMIF_TILE) * 2 + 64 * 4)
#include "vfo_fmif_kernels.h"
#include "vfo_rds_kernels.h"
#include "vfo_stereo_kernels.h"
#include "vfo_sym_kernels.h"
#include "vfo_rdsd_kernels.h"
#include "vfo_qpsk_kernels.h"
#include "vfo_frame_kernels.h"

namespace sdrpp_k {

static_assert(SDRPP_FMIF_LDS_FLOATS <= SDRPP_WAVE_LDS_FLOATS, "FMIF: window and exchange");
static_assert(SDRPP_ST_PILOT_TILE + SDRPP_ST_PILOT_MAX_TAPS <= SDRPP_WAVE_LDS_FLOATS, "stereo pilot: phases of a tile and the taps in front of it");
static_assert(2 * (SDRPP_ST_MATRIX_TILE + SDRPP_ST_AUDIO_MAX_TAPS - 1) <= SDRPP_WAVE_LDS_FLOATS, "stereo matrix: two windows");
static_assert(SDRPP_ST_LOOP_PTRS + SDRPP_ST_LOOP_CHUNK + SDRPP_ST_PACK <= SDRPP_WAVE_LDS_FLOATS, "stereo loop: the rows of a chunk");
static_assert(SDRPP_SYM_TILE + SDRPP_SYM_MAX_SHAPE_TAPS <= SDRPP_WAVE_LDS_FLOATS, "symbol front: phases of a tile and the taps in front of it");
static_assert(!wave_kind_uses_lds(WK_SYM_LOOP), "symbol loop: no LDS");
static_assert(SDRPP_RDSD_LDS_FLOATS <= SDRPP_WAVE_LDS_FLOATS && wave_kind_uses_lds(WK_RDS_DEMOD), "RDS demodulator: the filter's window of a chunk and MM's work buffer");
static_assert(SDRPP_QPSK_FRONT_LDS_FLOATS <= SDRPP_WAVE_LDS_FLOATS && wave_kind_uses_lds(WK_QPSK_FRONT), "QPSK front: the window of a tile");
static_assert(SDRPP_QPSK_LOOP_LDS_FLOATS <= SDRPP_WAVE_LDS_FLOATS && wave_kind_uses_lds(WK_QPSK_LOOP), "QPSK loop: MM's work buffer of a chunk");
static_assert(SDRPP_FRAME_LDS_FLOATS <= SDRPP_WAVE_LDS_FLOATS && wave_kind_uses_lds(WK_SYM_FRAME), "framer: a chunk's bit words, its match mask, the push ends and the frame under construction");
// (the RDS front's window depends on its filter: the host admits only a tile whose window and phases fit the stride, rds_tile_geometry)

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
// One record per VFO (WK_NBSQ).
struct NbSqJob {
    const float2* in;  // the IF stream of this push (RxVFO::out)
    float2* out;       // the chain's own output
    float* amp;        // NoiseBlanker::amp, persistent (device)
    int n;
    int nb_on;
    float nb_rate, nb_inv_rate, nb_level;
    int sq_on;
    float sq_level;
    // reference blocks inside this push at the IF rate (cumulative sample counts; nullptr: the push is one block)
    const int* bounds;
    int nb;
};
__device__ __forceinline__ void vfo_nbsq_body(const NbSqJob& job) {
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
// wavefront `id` of the role: its entry of the table says what it is.  The entry and every record are read with scalar loads (wave_uniform_job, here and in
// the `*_call`s): a record in scalar registers costs a wavefront one short round trip behind its entry, where vector loads cost FMIF's short segment jobs 1 to 2 %
// of a tick (profiles/wave_jobs_ab.md).  The two bodies of this header are inlined, as they were; the others are calls.
__device__ __forceinline__ void vfo_wave_body(int id, const WaveJob* __restrict__ jobs, float* smem) {
    const WaveJob job = wave_uniform_job(jobs + id);
    switch (job.kind) {
    case WK_NBSQ: vfo_nbsq_body(wave_uniform_job(static_cast<const NbSqJob*>(job.rec))); break;
    case WK_FMIF: vfo_fmif_body(wave_uniform_job(static_cast<const FmifJob*>(job.rec)), job.arg, smem); break;
    case WK_RDS_FRONT: vfo_rds_front_call(static_cast<const RdsJob*>(job.rec), smem); break;
    case WK_RDS_ROTX: vfo_rds_rotate_exact_call(static_cast<const RdsRotXJob*>(job.rec)); break;
    case WK_RDS_LINE: vfo_rds_line_call(static_cast<const RdsLineJob*>(job.rec)); break;
    case WK_ST_PILOT: vfo_stereo_pilot_call(static_cast<const StereoPilotJob*>(job.rec), smem); break;
    case WK_ST_LOOP: vfo_stereo_loop_call(static_cast<const StereoLoopJob*>(job.rec), smem); break;
    case WK_ST_MATRIX: vfo_stereo_matrix_call(static_cast<const StereoMatrixJob*>(job.rec), smem); break;
    case WK_SYM_FRONT: vfo_sym_front_call(static_cast<const SymFrontJob*>(job.rec), smem); break;
    case WK_SYM_LOOP: vfo_sym_loop_call(static_cast<const SymLoopJob*>(job.rec)); break;
    case WK_RDS_DEMOD: vfo_rdsd_call(static_cast<const RdsdJob*>(job.rec), smem); break;
    case WK_QPSK_FRONT: vfo_qpsk_front_call(static_cast<const QpskFrontJob*>(job.rec), job.arg, smem); break;
    case WK_QPSK_LOOP: vfo_qpsk_loop_call(static_cast<const QpskLoopJob*>(job.rec), smem); break;
    case WK_SYM_FRAME: vfo_sym_frame_call(static_cast<const FrameJob*>(job.rec), smem); break;
    default: break;
    }
}
// four jobs per workgroup, one per wavefront (gx = ceil(njobs / 4)): the shape the role has inside a tick.  LDS: 4 * SDRPP_WAVE_LDS_FLOATS floats where
// the table holds a kind that uses it (wave_kind_uses_lds), none otherwise.
__global__ __launch_bounds__(256) void vfo_ifchain_kernel(const WaveJob* __restrict__ jobs, int njobs) {
    HIP_DYNAMIC_SHARED(float, smemi)
    const int j = (int)blockIdx.x * 4 + ((int)threadIdx.x >> 6);
    if (j < njobs) { vfo_wave_body(j, jobs, smemi); }
}

}  // namespace sdrpp_k
