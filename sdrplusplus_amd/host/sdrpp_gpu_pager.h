// POCSAGDSP-shaped adaptor for the pager decoder (decoder_modules/pager_decoder/src/pocsag/dsp.h:14-76, decoder.h).
//
// In the reference the pager decoder owns a VFO and, behind its output stream, a POCSAGDSP block with a thread of its own: Quadrature(-4500 Hz) ->
// FIR<float, float> -> clock_recovery::MM<float> -> BinarySlicer, with `out` (one bit per symbol) and `soft` (the soft symbols; swapped only for a block that
// produced some, dsp.h:63).  On the GPU that chain is the symbol branch of the channel itself (sdrpp_vfo_set_symbols), inside the VFO bank: the object the
// decoder holds does no signal processing of its own.  init() finds the sdrpp_gpu::RxVFO whose `out` stream it is handed as `in`, attaches the branch to it
// (RxVFO::attachSymbols) and `out` / `soft` are that channel's symbol streams, filled by the front end's worker — block by block or, with
// IQFrontEnd::setPipelining, out of every block's result slot.  One front end serves every pager channel of a capture.
//
//   #include <sdrpp_gpu_pager.h>
//   sdrpp_gpu::POCSAGDSP dsp(&sigpath::iqFrontEnd);
//   dsp.init(vfo->output, 24000, 2400);                       // pocsag/decoder.h:20: dsp.init(vfo->output, 24000, baudrate)
//   reshape.init(&dsp.soft, 2400.0, (2400 / 30.0) - 2400.0);  // decoder.h:21-23, unchanged
//   dataHandler.init(&dsp.out, _dataHandler, this);
//
// start() / stop() have no counterpart (the front end's cover them); they are kept so that the decoder's call sequence stays valid.  The channel must deliver
// its IF (no demodulator attached) at the sample rate init() is given.
#pragma once
#include <stdexcept>

#include "sdrpp_gpu_blocks.h"

namespace sdrpp_gpu {

class POCSAGDSP {
public:
    explicit POCSAGDSP(IQFrontEnd* frontEnd) : out(dummyOut), soft(dummySoft), fe(frontEnd) {}
    POCSAGDSP(IQFrontEnd* frontEnd, dsp::stream<dsp::complex_t>* in, double samplerate, double baudrate) : POCSAGDSP(bound(frontEnd, in), frontEnd, samplerate, baudrate) {}
    ~POCSAGDSP() {
        if (vfo && fe && fe->vfoOfStream(&vfo->out) == vfo) { vfo->detachSymbols(); }
    }
    POCSAGDSP(const POCSAGDSP&) = delete;
    POCSAGDSP& operator=(const POCSAGDSP&) = delete;

    // As the reference's: `in` is the VFO's output stream.  A block whose streams are members cannot re-seat them, so an object built with the one-argument
    // constructor is bound by init() to the channel and its `out` / `soft` are reached through output() / softOutput(); the four-argument constructor (the
    // reference's POCSAGDSP(in, samplerate, baudrate)) binds at once and `out` / `soft` ARE the channel's streams.
    void init(dsp::stream<dsp::complex_t>* in, double samplerate, double baudrate) {
        RxVFO* v = bound(fe, in);
        if (vfo && vfo != v) { vfo->detachSymbols(); }
        vfo = v;
        attach(samplerate, baudrate);
    }
    void setBaudrate(double baudrate) {  // (dsp.h:47-53 leaves it empty; here it re-attaches: the loop starts over at the new rate)
        if (vfo) { vfo->attachSymbols(baudrate); }
    }
    void start() {}
    void stop() {}
    dsp::stream<uint8_t>* output() { return vfo ? &vfo->symOut : nullptr; }
    dsp::stream<float>* softOutput() { return vfo ? &vfo->symSoft : nullptr; }
    RxVFO* channel() { return vfo; }

    dsp::stream<uint8_t>& out;
    dsp::stream<float>& soft;

private:
    POCSAGDSP(RxVFO* v, IQFrontEnd* frontEnd, double samplerate, double baudrate) : out(v->symOut), soft(v->symSoft), fe(frontEnd), vfo(v) { attach(samplerate, baudrate); }
    static RxVFO* bound(IQFrontEnd* frontEnd, dsp::stream<dsp::complex_t>* in) {
        RxVFO* v = frontEnd ? frontEnd->vfoOfStream(in) : nullptr;
        if (!v) { throw std::runtime_error("[sdrpp_gpu::POCSAGDSP] the input is not the output stream of a VFO of this front end (the decoder's DSP is fused behind the channeliser)"); }
        return v;
    }
    void attach(double samplerate, double baudrate) {
        if (vfo->demod != Demod::RAW) { throw std::runtime_error("[sdrpp_gpu::POCSAGDSP] the channel carries a demodulator: the pager reads the VFO's IF"); }
        if (vfo->outSamplerate != samplerate) { throw std::runtime_error("[sdrpp_gpu::POCSAGDSP] the channel does not run at the sample rate the decoder was given"); }
        vfo->attachSymbols(baudrate);
    }

    dsp::stream<uint8_t> dummyOut;   // what `out` / `soft` name until a channel is bound (the one-argument constructor): never written
    dsp::stream<float> dummySoft;
    IQFrontEnd* fe;
    RxVFO* vfo = nullptr;
};

}  // namespace sdrpp_gpu
