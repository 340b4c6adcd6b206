// History carry of the streams, and the gather of the per-VFO outputs of a push.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <sdrpp_gfx950.h>
#include "fft_kernels.h"

namespace sdrpp_k {

// =====================================================================================================================
// History carry: after a push of n samples, the new history of a stream is the last hist_len samples of (old history ++ data).
// Written to the stream's alternate history buffer (ping-pong), so the update is race-free for any n.
// =====================================================================================================================
struct CarryJob {
    const float* data;
    const float* old_hist;
    float* new_hist;
    int hist_len, n, width;
    int need;  // only the most recent `need` samples will be read by the next push: older entries are not copied
};
// njw > 0: ONE WAVEFRONT per job (job 4 bid.y + wavefront of njw) — the per-VFO histories are a few hundred samples, a workgroup's life is
// the chain of round trips to its job and back whatever it moves, and in a tick workgroup SLOTS are what the roles compete for (cfg 4:
// 1 300-1 500 carry workgroups of 4.5 us were an eighth of the tick's slot time); njw = 0: grid.x workgroups stride over job bid.y.
__device__ __forceinline__ void carry_body(const KIdx bid, const KIdx gdim, const CarryJob* __restrict__ jobs, int njw) {
    const int jidx = njw > 0 ? bid.y * 4 + ((int)threadIdx.x >> 6) : bid.y;
    if (njw > 0 && jidx >= njw) { return; }
    const CarryJob job = jobs[jidx];
    const int first = (job.hist_len - job.need) * job.width;
    const int total = job.hist_len * job.width;
    // new_hist[e] = (old_hist ++ data)[n * width + e]: elements below `eb` still come from the old history (a push shorter than the history),
    // the rest from the data of this push at data[e - eb]
    const long long nw = (long long)job.n * job.width;
    const long long ebl = (long long)total - nw;
    const int eb = ebl < 0 ? 0 : (ebl > total ? total : (int)ebl);
    // Round 5: FOUR floats per access (one dwordx4 load / store, 4-byte alignment is all global memory asks for) and eight accesses in flight per
    // work-item before the first store — the carries of a tick were thousands of workgroups of one 4-byte load per work-item each (cfg 4: ~2 300
    // workgroups of 3.9 us, the whole tail of the tick), their life a memory round trip whatever they carry: fewer, fatter workgroups.
    const int first4 = (first + 3) & ~3;
    const int nthreads = njw > 0 ? 64 : gdim.x * 256, t = njw > 0 ? ((int)threadIdx.x & 63) : bid.x * 256 + (int)threadIdx.x;
    for (int e = first + t; e < first4 && e < total; e += nthreads) {  // (the up to three elements in front of the first whole quad)
        const long long sx = nw + e;
        global_store_f32_boff(job.new_hist, (unsigned)e * 4u, global_load_f32(e < eb ? job.old_hist : job.data, e < eb ? sx : (long long)e - ebl));
    }
    constexpr int U = 8;
    for (int q0 = first4 + 4 * t; q0 < total; q0 += 4 * nthreads * U) {
        float4 v[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            int e = q0 + 4 * nthreads * u;
            if (e >= total) { e = first4; }  // (beyond the end: some quad that exists — never a guarded load; nothing is stored for it below)
            if (e + 3 < eb) { v[u] = global_load_f32x4_unaligned(job.old_hist, nw + e); }
            else if (e >= eb && e + 3 < total) { v[u] = global_load_f32x4_unaligned(job.data, (long long)e - ebl); }
            else {  // the quad that straddles the seam between the two sources, or the last, partial one: element by element
                float w4[4];
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const int ek = e + k < total ? e + k : total - 1;
                    w4[k] = global_load_f32(ek < eb ? job.old_hist : job.data, ek < eb ? nw + ek : (long long)ek - ebl);
                }
                v[u] = make_float4(w4[0], w4[1], w4[2], w4[3]);
            }
        }
#pragma unroll
        for (int u = 0; u < U; u++) {
            const int e = q0 + 4 * nthreads * u;
            if (e + 3 < total) { global_store_f32x4_unaligned(job.new_hist, e, v[u]); }
            else if (e < total) {  // the last, partial quad
                const float w4[4] = { v[u].x, v[u].y, v[u].z, v[u].w };
                for (int k = 0; k < 4 && e + k < total; k++) { global_store_f32_boff(job.new_hist, (unsigned)(e + k) * 4u, w4[k]); }
            }
        }
    }
}
__global__ __launch_bounds__(256) void carry_kernel(const CarryJob* __restrict__ jobs, int njw) { carry_body(kidx(blockIdx), kidx(gridDim), jobs, njw); }

// =====================================================================================================================
// Output gather (sdrpp_vfo_read_many): the per-VFO output blocks of one push packed back to back, so that the host gets all of them
// with ONE device-to-host copy instead of one small copy (and stream synchronisation) per VFO.
// =====================================================================================================================
struct GatherJob {
    const float2* src;
    long long dst_off;  // samples
    int n;
};
__global__ __launch_bounds__(256) void gather_kernel(const GatherJob* __restrict__ jobs, float2* __restrict__ dst) {
    const GatherJob job = jobs[blockIdx.y];
    for (int i = (int)(blockIdx.x * blockDim.x + threadIdx.x); i < job.n; i += (int)(gridDim.x * blockDim.x)) { dst[job.dst_off + i] = job.src[i]; }
}
// the same with the job table in the kernel arguments (up to 128 VFOs: 3 KB of the 4 KB the launch packet carries): no upload of the table,
// which for a read after every reference-sized block was a staged host-to-device copy of its own
#define SDRPP_GATHER_INLINE 128
struct GatherArgs { GatherJob j[SDRPP_GATHER_INLINE]; };
__global__ __launch_bounds__(256) void gather_inline_kernel(GatherArgs args, float2* __restrict__ dst) {
    const GatherJob job = args.j[blockIdx.y];
    for (int i = (int)(blockIdx.x * blockDim.x + threadIdx.x); i < job.n; i += (int)(gridDim.x * blockDim.x)) { dst[job.dst_off + i] = job.src[i]; }
}

}  // namespace sdrpp_k
