// Converting landing copy: the wire formats of the reference's sources (include/sdrpp_gpu.h: SDRPP_IQ_I8 / _I16 / _U8) -> the float landing
// buffer, so that the bus carries 2 (8-bit) or 4 (16-bit) bytes per complex sample instead of 8.  Feed-forward, no streaming state, every value
// exactly specified:
//     I8 / I16   (float)x * inv      inv = 1.0f / scalar, ONE float division on the host; the conversion int -> float of an 8- or 16-bit integer is
//                                    exact, the product is one float multiply (volk_8i_s32f_convert_32f / volk_16i_s32f_convert_32f, generic)
//     U8         table[b]            256 floats the host computed in the source's own arithmetic (sdrpp_design_u8_table); the device only looks up
// One routine, two callers: the tick's landing copy (tick_kernels.h: CopyJob kind 4, source = page-locked host memory) and ingest_kernel behind
// the raw H2D copy of an ordinary / deferred pass.
#pragma once

namespace sdrpp_k {

enum IngestType : int { ING_I8 = 0, ING_I16 = 1, ING_U8 = 2 };

// one value out of the dword it lies in (little endian; `sh` = its bit offset: 0 / 8 / 16 / 24, 16-bit values 0 / 16)
template <int T>
__device__ __forceinline__ float ingest_value(unsigned w, int sh, float inv, const float* table) {
    if constexpr (T == ING_I16) { return (float)((int)(w << (16 - sh)) >> 16) * inv; }
    else if constexpr (T == ING_I8) { return (float)((int)(w << (24 - sh)) >> 24) * inv; }
    else { return global_load_f32(table, (long long)((w >> sh) & 0xffu)); }
}
// the values of one dword, in memory order -> d[0 .. 4) (8-bit) / d[0 .. 2) (16-bit)
template <int T>
__device__ __forceinline__ void ingest_word(unsigned w, float inv, const float* table, float* d) {
    if constexpr (T == ING_I16) {
        d[0] = ingest_value<T>(w, 0, inv, table);
        d[1] = ingest_value<T>(w, 16, inv, table);
    }
    else {
        d[0] = ingest_value<T>(w, 0, inv, table);
        d[1] = ingest_value<T>(w, 8, inv, table);
        d[2] = ingest_value<T>(w, 16, inv, table);
        d[3] = ingest_value<T>(w, 24, inv, table);
    }
}
// one 16-byte source vector -> 16 (8-bit) / 8 (16-bit) floats at `out` (4-byte aligned at least: a global store needs no more), in 16-byte stores
template <int T>
__device__ __forceinline__ void ingest_vector(const uint4 v, float inv, const float* table, float* out) {
    const unsigned w[4] = { v.x, v.y, v.z, v.w };
    if constexpr (T == ING_I16) {
#pragma unroll
        for (int q = 0; q < 2; q++) {
            float d[4];
            ingest_word<T>(w[2 * q], inv, table, d);
            ingest_word<T>(w[2 * q + 1], inv, table, d + 2);
            global_store_f32x4_unaligned(out, 4 * q, make_float4(d[0], d[1], d[2], d[3]));
        }
    }
    else {
#pragma unroll
        for (int q = 0; q < 4; q++) {
            float d[4];
            ingest_word<T>(w[q], inv, table, d);
            global_store_f32x4_unaligned(out, 4 * q, make_float4(d[0], d[1], d[2], d[3]));
        }
    }
}

// `bytes` source bytes at `src` (any SAMPLE boundary: 2-byte aligned for the 8-bit formats, 4-byte for I16 — the second push of a launch group starts
// right behind a 7-sample one) -> floats at `dst`; work-item `tid` of `nth`.
//  - 16-byte loads from the first 16-byte boundary of the source on, EIGHT in flight per work-item before the first store: out of page-locked host
//    memory every load is a round trip over the bus, and few workgroups with many loads each disturb fewer CUs than many with one (the verbatim
//    copy's shape, tick_kernels.h copy_one, for the reason given there);
//  - the values in front of that boundary and behind the last whole vector go out one per work-item.  They are read as the ALIGNED dword they lie
//    in: at most two bytes in front of the first / behind the last value, inside the buffers the host side owns (staging slots and raw landing
//    buffers start 16-byte aligned and end in spare room) — a copy from the caller's own memory would not be entitled to that.
// Explicit global loads / stores throughout (sdrpp_gfx950.h: through the generic pointers every access was flat and the in-flight vectors lived in
// scratch).  No atomics, vector stores only.
template <int T>
__device__ __forceinline__ void ingest_convert(const void* src, float* dst, long long bytes, float inv, const float* table, long long tid, long long nth) {
    constexpr int BPV = T == ING_I16 ? 2 : 1;  // bytes per value
    constexpr int VPV = 16 / BPV;              // values per 16-byte vector
    const unsigned long long a0 = (unsigned long long)src;
    long long head = (long long)((16ull - (a0 & 15ull)) & 15ull);  // bytes in front of the first 16-byte boundary
    if (head > bytes) { head = bytes; }
    const long long n16 = (bytes - head) / 16, tail = bytes - head - n16 * 16;
    const void* src16 = reinterpret_cast<const char*>(src) + head;
    float* dst16 = dst + head / BPV;
    constexpr int U = 8;
    long long i = tid;
    for (; i + (U - 1) * nth < n16; i += U * nth) {
        uint4 v[U];
#pragma unroll
        for (int u = 0; u < U; u++) { v[u] = global_load_u32x4(src16, i + u * nth); }
#pragma unroll
        for (int u = 0; u < U; u++) { ingest_vector<T>(v[u], inv, table, dst16 + (i + u * nth) * VPV); }
    }
    for (; i < n16; i += nth) { ingest_vector<T>(global_load_u32x4(src16, i), inv, table, dst16 + i * VPV); }
    const long long nh = head / BPV, nt = tail / BPV, nv = bytes / BPV;
    for (long long k = tid; k < nh + nt; k += nth) {
        const long long idx = k < nh ? k : nv - nt + (k - nh);
        const unsigned long long a = a0 + (unsigned long long)idx * BPV;
        const unsigned w = global_load_u32(reinterpret_cast<const void*>(a & ~3ull), 0);
        global_store_u32(dst, idx, __float_as_uint(ingest_value<T>(w, (int)(a & 3ull) * 8, inv, table)));
    }
}
__device__ __forceinline__ void ingest_body(const void* src, float* dst, long long bytes, int type, float inv, const float* table, long long tid, long long nth) {
    // (uniform over the launch)
    if (type == ING_I16) { ingest_convert<ING_I16>(src, dst, bytes, inv, table, tid, nth); }
    else if (type == ING_I8) { ingest_convert<ING_I8>(src, dst, bytes, inv, table, tid, nth); }
    else { ingest_convert<ING_U8>(src, dst, bytes, inv, table, tid, nth); }
}
// (a call, not inlined, where the tick kernel uses it: its three conversion loops would otherwise take part in that kernel's register allocation, as the
// recorder's did — rec_body_call, tick_kernels.h)
__device__ __attribute__((noinline)) void ingest_body_call(const void* src, float* dst, long long bytes, int type, float inv, const float* table, int bx, int gx) {
    ingest_body(src, dst, bytes, type, inv, table, (long long)bx * 256 + threadIdx.x, (long long)gx * 256);
}
// ordinary and deferred passes: the raw block has been copied to device memory as it came; grid of 256-thread workgroups
__global__ __launch_bounds__(256) void ingest_kernel(const void* __restrict__ src, float* __restrict__ dst, long long bytes, int type, float inv, const float* __restrict__ table) {
    ingest_body(src, dst, bytes, type, inv, table, (long long)blockIdx.x * 256 + threadIdx.x, (long long)gridDim.x * 256);
}

}  // namespace sdrpp_k
