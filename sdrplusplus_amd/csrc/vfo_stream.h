// A VFO's streams between the stages: this push's samples and the history in front of them, and the four loaders.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <sdrpp_gfx950.h>

namespace sdrpp_k {

// A stream of `width`-float samples: this push's samples in `data`, the previous `hist_len` samples in `hist`.
struct StreamIn {
    const float* data;
    const float* hist;
    int hist_len;
    int n;  // valid samples in `data`
};
__device__ __forceinline__ float2 stream_load2(const StreamIn& s, int i) {
    const float2* d = reinterpret_cast<const float2*>(s.data);
    const float2* h = reinterpret_cast<const float2*>(s.hist);
    if (i >= s.n) { return make_float2(0.0f, 0.0f); }  // tile over-read past the end of this push
    return (i >= 0) ? global_load_f32x2(d, i) : global_load_f32x2(h, s.hist_len + i);  // (explicit GLOBAL loads: a plain dereference of a job-table pointer is FLAT)
}
__device__ __forceinline__ float stream_load1(const StreamIn& s, int i) {
    if (i >= s.n) { return 0.0f; }
    return (i >= 0) ? global_load_f32(s.data, i) : global_load_f32(s.hist, s.hist_len + i);
}
// The same without a branch, for loops that fetch several samples per lane: the load is unconditional (the address is clamped into the
// stream, the value selected afterwards), so the compiler issues all loads of the loop before the first wait — behind a per-element
// branch every load costs its own memory round trip (measured: 18 x 0.75 us for the first window of the audio filter of a 50 000-sample
// block).  Same values; needs i >= -hist_len like the functions above.
__device__ __forceinline__ float2 stream_load2_nb(const StreamIn& s, int i, bool ok = true) {  // ok false: zero (no load is ever guarded by a branch)
    const bool use = ok && i < s.n, cur = i >= 0;
    int ic = cur ? i : (s.hist_len + i);
    ic = (use && ic >= 0) ? ic : 0;
    const float2 v = global_load_f32x2(reinterpret_cast<const float2*>((cur || !use) ? s.data : s.hist), ic);  // (not wanted: element 0 of the data buffer, which always exists)
    return use ? v : make_float2(0.0f, 0.0f);
}
__device__ __forceinline__ float stream_load1_nb(const StreamIn& s, int i, bool ok = true) {
    const bool use = ok && i < s.n, cur = i >= 0;
    int ic = cur ? i : (s.hist_len + i);
    ic = (use && ic >= 0) ? ic : 0;
    const float v = global_load_f32((cur || !use) ? s.data : s.hist, ic);
    return use ? v : 0.0f;
}

}  // namespace sdrpp_k
