// Per-VFO channeliser + demodulator kernels for gfx950.
//
// Reference data flow per VFO and per input block (core/src/dsp/channel/rx_vfo.h:89-100):
//   FrequencyXlator (VOLK rotator, full input rate)  ->  PowerDecimator cascade of DecimatingFIR stages
//   (dsp/filter/decimating_fir.h:45-68)  ->  PolyphaseResampler (dsp/multirate/polyphase_resampler.h:69-99)  ->
//   channel FIR (dsp/filter/fir.h:62-83)  ->  demodulator (dsp/demod/{quadrature,fm,broadcast_fm,am,ssb}.h).
// The reference runs one thread per block and one VOLK dot product per output sample; every VFO re-reads its own copy of
// the input (Splitter memcpy).  Here the time axis is split across workgroups (each stream keeps the (taps-1)-sample
// history of its consumer in a small side buffer, so results do not depend on how the input is cut into pushes), all
// VFOs of a launch are processed by the same grid, and the full-rate stage reads the shared IQ buffer once per tile.
//
// Numerics: summation order inside a dot product and the NCO differ from the reference's sequential fp32 recursion
// (VOLK's own SIMD kernels differ from its generic ones in the same way); parity is by tolerance (1e-5 RMS), see DESIGN.md.
#pragma once
#include "vfo_math.h"
#include "vfo_stream.h"
#include "vfo_stage1_kernels.h"
#include "vfo_rot_kernels.h"
#include "vfo_resample_kernels.h"
#include "vfo_fir_kernels.h"
#include "vfo_demod_kernels.h"
#include "vfo_ifchain_kernels.h"  // (with the kinds of its role: vfo_fmif_kernels.h, vfo_rds_kernels.h, vfo_stereo_kernels.h, vfo_sym_kernels.h, vfo_frame_kernels.h)
#include "vfo_carry_kernels.h"
#include "vfo_af_kernels.h"
#include "vfo_rec_kernels.h"
#include "vfo_front_kernels.h"
#include "vfo_toep_kernels.h"
#include "vfo_polyc_kernels.h"  // (last, where vfo_polyc_kernel was defined before the split: the order of the kernels in the code object; it has no other meaning)
