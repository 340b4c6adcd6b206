// The front of the M17 decoder module (decoder_modules/m17_decoder/src/m17dsp.h: M17Decoder::init, :640-700) as one source of frames.
//
// In the reference M17Decoder is a hier_block: dsp::demod::GFSK (Quadrature(2400 Hz) -> 31 root-raised-cosine taps -> MM<float>), a doubler whose second output is
// `diagOut`, M17Slice4FSK and M17FrameDemux, each with a thread of its own; behind the demux's four streams sit M17LSFDecoder (linkSetupOut), M17LICHDecoder
// (lichOut), M17PayloadFEC -> M17Codec2Decode (streamOut) and a null sink (packetOut).  On the GPU everything up to and including the demux is the channel's
// symbol branch with the framer behind it (sdrpp_design_m17, sdrpp_vfo_set_symbols, sdrpp_vfo_set_framer), inside the VFO bank: the object the module holds does
// no signal processing of its own.  init() finds the sdrpp_gpu::RxVFO whose `out` stream it is handed, attaches the branch (RxVFO::attachM17) and offers the
// demux's streams, filled by the front end's worker — block by block or, with IQFrontEnd::setPipelining, out of every block's result slot (flags 64 and 512).
// The reference's decoders attach unchanged:
//
//   #include <sdrpp_gpu_m17.h>
//   sdrpp_gpu::M17FrameSource front(&sigpath::iqFrontEnd);
//   front.init(vfo->output, 14400);
//   decodeLSF.init(front.linkSetupOut(), handler, ctx);      // m17dsp.h: decodeLSF.init(&demux.linkSetupOut, ...)
//   decodeLICH.init(front.lichOut(), handler, ctx);
//   payloadFEC.init(front.streamOut());  decodeAudio.init(&payloadFEC.out, 8000);
//   ns.init(front.packetOut());  diagReshape.init(front.diagOut(), 480, 0);
//
// SWAP COUNTS are the reference's (m17dsp.h:208-221), one bit per byte: a link setup frame is one swap of 368 on linkSetupOut; a stream / packet frame is a swap
// of 96 on lichOut followed by a swap of 368 on streamOut / packetOut.  DEVIATION: the reference writes only 272 entries of those 368 and leaves the last 96 as
// whatever the buffer held before; here they are ZERO.  Nobody reads them (M17PayloadFEC reads 272).  diagOut carries the clock recovery's soft symbols, one swap
// per block that started any.  A frame is delivered with the block in which the reference's demux would have completed it.
// start() / stop() have no counterpart (the front end's cover them).  The channel must deliver its IF (no demodulator attached) at the rate init() is given.
#pragma once
#include <stdexcept>

#include "sdrpp_gpu_blocks.h"

namespace sdrpp_gpu {

class M17FrameSource {
public:
    explicit M17FrameSource(IQFrontEnd* frontEnd) : fe(frontEnd) {}
    ~M17FrameSource() {
        if (vfo && fe && fe->vfoOfStream(&vfo->out) == vfo) { vfo->detachM17(); }
    }
    M17FrameSource(const M17FrameSource&) = delete;
    M17FrameSource& operator=(const M17FrameSource&) = delete;

    // As M17Decoder::init(input, sampleRate, ...): `in` is the VFO's output stream
    void init(dsp::stream<dsp::complex_t>* in, double samplerate) {
        RxVFO* v = fe ? fe->vfoOfStream(in) : nullptr;
        if (!v) { throw std::runtime_error("[sdrpp_gpu::M17FrameSource] the input is not the output stream of a VFO of this front end (the decoder's front is fused behind the channeliser)"); }
        if (v->demod != Demod::RAW) { throw std::runtime_error("[sdrpp_gpu::M17FrameSource] the channel carries a demodulator: the M17 decoder reads the VFO's IF"); }
        if (v->outSamplerate != samplerate) { throw std::runtime_error("[sdrpp_gpu::M17FrameSource] the channel does not run at the sample rate the decoder was given"); }
        if (vfo && vfo != v) { vfo->detachM17(); }
        vfo = v;
        vfo->attachM17();
    }
    void start() {}
    void stop() {}
    dsp::stream<uint8_t>* linkSetupOut() { return vfo ? &vfo->m17LinkSetup : nullptr; }
    dsp::stream<uint8_t>* lichOut() { return vfo ? &vfo->m17Lich : nullptr; }
    dsp::stream<uint8_t>* streamOut() { return vfo ? &vfo->m17Stream : nullptr; }
    dsp::stream<uint8_t>* packetOut() { return vfo ? &vfo->m17Packet : nullptr; }
    dsp::stream<float>* diagOut() { return vfo ? &vfo->symSoft : nullptr; }
    RxVFO* channel() { return vfo; }

private:
    IQFrontEnd* fe;
    RxVFO* vfo = nullptr;
};

}  // namespace sdrpp_gpu
