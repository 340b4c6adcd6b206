// Recorder sink (misc_modules/recorder): what the recorder module does to a radio's audio stream, one block at a time —
//   dsp::audio::Volume (audio/volume.h:14,22,37: x * powf(volume, 2))  ->  dsp::bench::PeakLevelMeter<stereo_t> (bench/peak_level_meter.h:52-57)
//   ->  optionally dsp::convert::StereoToMono (convert/stereo_to_mono.h:13-15: (l + r) / 2.0f)
//   ->  wav::Writer::write in the file's sample type (utils/wav.cpp:158-180), with "ignore silence" (recorder/src/main.cpp:533-561).
// Every operation is an elementwise float32 product / sum or a maximum, so every output is a bit-exact function of the floats the stream holds:
// products and sums are rounded one by one (rec_mul / rec_add: nothing contracts into a fused multiply-add).
// One workgroup per job; a job is one VFO's share of a block (a push; in a launch group the frames of ONE push).  It runs as a plain kernel behind an
// ordinary pass (sdrpp_vfo_rec_read) and, in pipelined mode, as a job kind of the copy role (tick_kernels.h: CopyJob kind 3) one level behind the
// stream's producer, writing samples and the block's record straight into the page-locked result slot.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <sdrpp_gfx950.h>
#include "../../include/sdrpp_gpu.h"  // SDRPP_REC_*: the sample types (wav::SampleType, utils/wav.h:25-30)

namespace sdrpp_k {

struct RecJob {
    const float2* src;  // n stereo frames (8-byte aligned)
    void* dst;          // n * channels samples of the type; element aligned only (a share starts at any frame of the group's block), the block it lies in 16-byte aligned
    void* info;         // RecInfo (4-byte aligned)
    int n;
    float gain;         // powf(volume, 2), computed once on the host
    int mono, type, ignore_silence, pad;
};
// = sdrpp_rec_info (include/sdrpp_gpu.h; sdrpp_gpu.hip asserts the size)
struct RecInfo {
    int frames, channels, sample_type, silent;
    float peak_l, peak_r, abs_max;
};

#if defined(__HIPCC__)
__device__ __forceinline__ float rec_mul(float a, float b) { return __fmul_rn(a, b); }
__device__ __forceinline__ float rec_add(float a, float b) { return __fadd_rn(a, b); }
__device__ __forceinline__ void rec_store_u8(void* p, long long i, unsigned v) { ((unsigned char __attribute__((address_space(1)))*)(uintptr_t)p)[i] = (unsigned char)v; }
__device__ __forceinline__ void rec_store_u16(void* p, long long i, unsigned v) { ((unsigned short __attribute__((address_space(1)))*)(uintptr_t)p)[i] = (unsigned short)v; }
#else  // (the test emulator is built with -ffp-contract=off: a product and a sum stay two roundings)
static inline float rec_mul(float a, float b) { return a * b; }
static inline float rec_add(float a, float b) { return a + b; }
static inline void rec_store_u8(void* p, long long i, unsigned v) { ((unsigned char*)p)[i] = (unsigned char)v; }
static inline void rec_store_u16(void* p, long long i, unsigned v) { ((unsigned short*)p)[i] = (unsigned short)v; }
#endif

// the three maxima of a block; `v > m` never lets a NaN in, like the reference's loops
struct RecAcc { float pl, pr, am; };
__device__ __forceinline__ void rec_max(float& m, float v) {
    if (v > m) { m = v; }
}
// one float -> ES bytes of the file's sample type, in the low bits
template <int ES>
__device__ __forceinline__ unsigned rec_sample(float s) {
    if constexpr (ES == 1) {
        // (uint8_t)((s * 127.0f) + 128.0f), utils/wav.cpp:169: product, then sum, then truncation toward zero.  Outside [0, 256) the reference's cast is
        // undefined: saturated to 0 / 255 here
        const float t = rec_add(rec_mul(s, 127.0f), 128.0f);
        return t >= 255.0f ? 255u : (t > 0.0f ? (unsigned)(int)t : 0u);
    }
    else if constexpr (ES == 2) {
        // volk_32f_s32f_convert_16i, generic: product, clamp, rintf, cast (pack_convert_kernel's rule)
        float r = rec_mul(s, 32767.0f);
        if (r > 32767.0f) { r = 32767.0f; }
        else if (r < -32768.0f) { r = -32768.0f; }
        return (unsigned)(int)rintf(r) & 0xffffu;
    }
    else { return __float_as_uint(s); }
}
template <int ES>
__device__ __forceinline__ void rec_store(void* dst, long long e, unsigned bits) {
    if constexpr (ES == 1) { rec_store_u8(dst, e, bits); }
    else if constexpr (ES == 2) { rec_store_u16(dst, e, bits); }
    else { global_store_u32(dst, e, bits); }
}
// frame f through the volume and the meter
__device__ __forceinline__ float2 rec_volume(const RecJob& j, int f, RecAcc& a) {
    const float2 x = global_load_f32x2(j.src, f);
    const float2 v = make_float2(rec_mul(x.x, j.gain), rec_mul(x.y, j.gain));
    rec_max(a.pl, fabsf(v.x));
    rec_max(a.pr, fabsf(v.y));
    return v;
}
__device__ __forceinline__ float rec_mono(float2 v, RecAcc& a) {
    const float m = rec_add(v.x, v.y) / 2.0f;
    rec_max(a.am, fabsf(m));
    return m;
}

// The samples of one job.  The destination is written in 16-byte vectors from its first 16-byte boundary on, FPC frames per work-item and vector; the
// frames in front of that boundary and behind the last whole vector go out one per work-item, element by element.  A frame is an 8-byte load: the
// source of a share is frame aligned and no more.
template <int ES, bool MONO>
__device__ __forceinline__ void rec_convert(const RecJob& j, RecAcc& a) {
    constexpr int CH = MONO ? 1 : 2, BPF = ES * CH, FPC = 16 / BPF;
    const int t = (int)threadIdx.x, n = j.n;
    const unsigned mis = (unsigned)((unsigned long long)(uintptr_t)j.dst & 15ull);  // (a multiple of BPF: the block starts on a 16-byte boundary)
    const int head = min((int)(((16u - mis) & 15u) / (unsigned)BPF), n);
    const int nvec = (n - head) / FPC, tail = head + nvec * FPC;
    const int f = t < head ? t : tail + (t - head);  // (fewer than 16 frames at either end)
    if (f < n) {
        const float2 v = rec_volume(j, f, a);
        if constexpr (MONO) { rec_store<ES>(j.dst, f, rec_sample<ES>(rec_mono(v, a))); }
        else {
            rec_store<ES>(j.dst, 2ll * f, rec_sample<ES>(v.x));
            rec_store<ES>(j.dst, 2ll * f + 1, rec_sample<ES>(v.y));
        }
    }
    void* const body = reinterpret_cast<char*>(j.dst) + (size_t)head * BPF;
    for (int c = t; c < nvec; c += 256) {
        unsigned w[4] = { 0u, 0u, 0u, 0u };
#pragma unroll
        for (int k = 0; k < FPC; k++) {
            const float2 v = rec_volume(j, head + c * FPC + k, a);
            if constexpr (MONO) { w[(k * ES) >> 2] |= rec_sample<ES>(rec_mono(v, a)) << (8 * ((k * ES) & 3)); }
            else {
                w[(2 * k * ES) >> 2] |= rec_sample<ES>(v.x) << (8 * ((2 * k * ES) & 3));
                w[((2 * k + 1) * ES) >> 2] |= rec_sample<ES>(v.y) << (8 * (((2 * k + 1) * ES) & 3));
            }
        }
        uint4 q;
        q.x = w[0];
        q.y = w[1];
        q.z = w[2];
        q.w = w[3];
        global_store_u32x4(body, c, q);
    }
}

// sm: 12 floats of LDS.  Every work-item of the 256 takes part (a barrier and wavefront-wide maxima inside).
__device__ __forceinline__ void rec_body(const RecJob& j, float* sm) {
    RecAcc a{ 0.0f, 0.0f, 0.0f };
    const bool mono = j.mono != 0;
    switch (j.type) {
    case SDRPP_REC_UINT8:
        if (mono) { rec_convert<1, true>(j, a); }
        else { rec_convert<1, false>(j, a); }
        break;
    case SDRPP_REC_INT16:
        if (mono) { rec_convert<2, true>(j, a); }
        else { rec_convert<2, false>(j, a); }
        break;
    default:
        if (mono) { rec_convert<4, true>(j, a); }
        else { rec_convert<4, false>(j, a); }
        break;
    }
    if (!mono) { a.am = a.pl > a.pr ? a.pl : a.pr; }  // what is written is the volume's output itself
    const float pl = wave_max(a.pl), pr = wave_max(a.pr), am = wave_max(a.am);
    const int w = (int)threadIdx.x >> 6;
    if (((int)threadIdx.x & 63) == 0) {
        sm[w * 3] = pl;
        sm[w * 3 + 1] = pr;
        sm[w * 3 + 2] = am;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        RecAcc r{ sm[0], sm[1], sm[2] };
        for (int k = 1; k < 4; k++) {
            rec_max(r.pl, sm[k * 3]);
            rec_max(r.pr, sm[k * 3 + 1]);
            rec_max(r.am, sm[k * 3 + 2]);
        }
        // recorder/src/main.cpp:28,543,557: ignoringSilence = absMax < SILENCE_LVL, a float against the double 10e-6; an empty block is never silent
        const int silent = (j.n > 0 && j.ignore_silence && (double)r.am < 10e-6) ? 1 : 0;
        global_store_u32(j.info, 0, (unsigned)j.n);
        global_store_u32(j.info, 1, mono ? 1u : 2u);
        global_store_u32(j.info, 2, (unsigned)j.type);
        global_store_u32(j.info, 3, (unsigned)silent);
        global_store_u32(j.info, 4, __float_as_uint(r.pl));
        global_store_u32(j.info, 5, __float_as_uint(r.pr));
        global_store_u32(j.info, 6, __float_as_uint(r.am));
    }
}

// behind an ordinary pass: one job, handed over by value
__global__ __launch_bounds__(256) void vfo_rec_kernel(RecJob job) {
    __shared__ float sm[12];
    rec_body(job, sm);
}

}  // namespace sdrpp_k
