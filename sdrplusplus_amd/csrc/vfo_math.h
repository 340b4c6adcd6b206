// Arithmetic idioms of the VFO kernels.  Operand and rounding order are part of every definition: the parity tests compare against the
// reference's own order, and the CPU emulator and the device must round alike.
// Each helper is used only where the compiler emits the same machine code as for the expression written out.  The NCO phasor (turn_sincos /
// turn_phasor) is that at all of its sites.  The others are not: cmul / cmul_re / cabs_ref serve vfo_rotate_body and vfo_demod_pre_body, cmac
// the resamplers and the VALU FIR forms, and these sites DELIBERATELY keep the inline expression, because calling the helper there changed
// instruction selection, scheduling or register allocation of the kernel (and of the tick kernel that holds it as a role):
//   |x| and the AGC's clamped gain in vfo_sequential_body, |x| in vfo_nbsq_body and vfo_fmif_body;
//   the complex multiply and the real-tap MAC in the stage-1 epilogues, vfo_front2_body and the matrix front ends' epilogues;
//   the tap-pair FMA quad in stage1_accumulate, stage1_accumulate_static and vfo_stage1_direct_body.
// Converting one of them is a change of device code: compare the disassembly and re-measure the kernel, it is not a clean-up.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <sdrpp_gfx950.h>

namespace sdrpp_k {

// sin / cos of a phase given in TURNS (double: the closed-form NCO, phi0 + n * theta): wrapped to +-0.5 turn, then evaluated in float.
__device__ __forceinline__ void turn_sincos(double turns, float& sn, float& cs) {
    double ph = turns;
    ph -= rint(ph);
    sincospif(2.0f * (float)ph, &sn, &cs);
}
// the phasor itself, (cos, sin)
__device__ __forceinline__ float2 turn_phasor(double turns) {
    float sn, cs;
    turn_sincos(turns, sn, cs);
    return make_float2(cs, sn);
}

// a * (cs + j sn)
__device__ __forceinline__ float cmul_re(float2 a, float cs, float sn) { return fmaf(a.x, cs, -(a.y * sn)); }
__device__ __forceinline__ float2 cmul(float2 a, float cs, float sn) { return make_float2(cmul_re(a, cs, sn), fmaf(a.x, sn, a.y * cs)); }

// acc += h * x, real tap on a complex sample
__device__ __forceinline__ void cmac(float h, float2 x, float2& acc) {
    acc.x = fmaf(h, x.x, acc.x);
    acc.y = fmaf(h, x.y, acc.y);
}

// |x| in the reference's order (volk_32fc_magnitude_32f: the squares are rounded, summed, then the root)
__device__ __forceinline__ float cabs_ref(float2 x) { return sqrtf((x.x * x.x) + (x.y * x.y)); }

}  // namespace sdrpp_k
