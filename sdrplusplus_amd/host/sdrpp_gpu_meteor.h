// dsp::demod::Meteor-shaped adaptor for the Meteor demodulator module (decoder_modules/meteor_demodulator/src/meteor_demod.h:9-197, main.cpp).
//
// In the reference the module owns a VFO and, behind its output stream, a dsp::demod::Meteor block with a thread of its own: root-raised-cosine FIR -> FastAGC ->
// MeteorCostas -> optional OQPSK delay -> MM<complex_t>, with `out` (one complex soft symbol per symbol); its sink turns every symbol into two int8 values.  On
// the GPU that chain is a block of the channel itself (sdrpp_vfo_set_qpsk): the object the module holds does no signal processing of its own.  init() finds the
// sdrpp_gpu::RxVFO whose `out` stream it is handed as `in`, attaches the demodulator to it (RxVFO::attachQPSK) and `out` is that channel's qpskOut stream, filled
// by the front end's worker — block by block or, with IQFrontEnd::setPipelining, out of every block's result slot (flag 256); packedOutput() is the channel's
// qpskPacked stream: the int8 pairs the module's sinkHandler would compute, made on the device (a swap carries 2 x the symbols).  From then on the channel's own
// `out` is no longer written: nobody reads it, and a dsp::stream without a reader blocks its writer.
//
//   #include <sdrpp_gpu_meteor.h>
//   sdrpp_gpu::Meteor demod(&sigpath::iqFrontEnd);
//   demod.init(&vfo->out, 72000.0f, 150000, 33, 0.6f, 0.1f, 0.005f, brokenModulation, oqpsk, 1e-6, 0.01);     // main.cpp:66
//   sink.init(demod.output(), sinkHandler, this);                                                               // or read demod.packedOutput() and write it out
//
// start() / stop() have no counterpart (the front end's cover them); they are kept so that the module's call sequence stays valid.  The module's setters that
// re-design the chain (setSymbolrate, setSamplerate, setRRCParams, setAGCRate, setCostasBandwidth, setMMParams, ...) are LEFT OUT: call init() again with the
// new values — it starts a fresh demodulator, as those setters' tempStop / re-design very nearly do.
#pragma once
#include <stdexcept>

#include "sdrpp_gpu_blocks.h"

namespace sdrpp_gpu {

class Meteor {
public:
    explicit Meteor(IQFrontEnd* frontEnd) : out(dummyOut), fe(frontEnd) {}
    // the reference's Meteor(in, symbolrate, ...): binds at once, `out` IS the channel's stream
    Meteor(IQFrontEnd* frontEnd, dsp::stream<dsp::complex_t>* in, double symbolrate, double samplerate, int rrcTapCount, double rrcBeta, double agcRate, double costasBandwidth,
           bool brokenModulation, bool oqpsk, double omegaGain, double muGain, double omegaRelLimit = 0.01)
        : Meteor(bound(frontEnd, in), frontEnd, RxVFO::QPSKParams{ symbolrate, samplerate, rrcTapCount, rrcBeta, agcRate, costasBandwidth, brokenModulation, oqpsk, omegaGain, muGain }) {
        (void)omegaRelLimit;
    }
    ~Meteor() {
        if (vfo && fe && fe->vfoOfStream(&vfo->out) == vfo) { vfo->detachQPSK(); }
    }
    Meteor(const Meteor&) = delete;
    Meteor& operator=(const Meteor&) = delete;

    // As the reference's (meteor_demod.h:24): `in` is the VFO's output stream.  omegaRelLimit is taken and, as in the reference, not passed on: MM keeps its default
    // 0.01.  A block whose streams are members cannot re-seat them, so an object built with the one-argument constructor is bound by init() and its streams are
    // reached through output() / packedOutput().  init() on a bound object moves it (the old channel delivers its `out` again) or, on the same channel, starts a
    // fresh demodulator.
    void init(dsp::stream<dsp::complex_t>* in, double symbolrate, double samplerate, int rrcTapCount, double rrcBeta, double agcRate, double costasBandwidth, bool brokenModulation, bool oqpsk,
              double omegaGain, double muGain, double omegaRelLimit = 0.01) {
        (void)omegaRelLimit;
        RxVFO* v = bound(fe, in);
        if (vfo && vfo != v) { vfo->detachQPSK(); }
        vfo = v;
        vfo->attachQPSK(RxVFO::QPSKParams{ symbolrate, samplerate, rrcTapCount, rrcBeta, agcRate, costasBandwidth, brokenModulation, oqpsk, omegaGain, muGain });
    }
    void setBrokenModulation(bool enabled) {
        if (vfo) { vfo->setQPSKMode(enabled, vfo->qpskP.oqpsk); }
    }
    void setOQPSK(bool enabled) {
        if (vfo) { vfo->setQPSKMode(vfo->qpskP.brokenModulation, enabled); }
    }
    void reset() {
        if (vfo) { vfo->resetQPSK(); }
    }
    void start() {}
    void stop() {}
    dsp::stream<dsp::complex_t>* output() { return vfo ? &vfo->qpskOut : nullptr; }
    dsp::stream<int8_t>* packedOutput() { return vfo ? &vfo->qpskPacked : nullptr; }
    RxVFO* channel() { return vfo; }

    dsp::stream<dsp::complex_t>& out;

private:
    Meteor(RxVFO* v, IQFrontEnd* frontEnd, const RxVFO::QPSKParams& p) : out(v->qpskOut), fe(frontEnd), vfo(v) { vfo->attachQPSK(p); }
    static RxVFO* bound(IQFrontEnd* frontEnd, dsp::stream<dsp::complex_t>* in) {
        RxVFO* v = frontEnd ? frontEnd->vfoOfStream(in) : nullptr;
        if (!v) { throw std::runtime_error("[sdrpp_gpu::Meteor] the input is not the output stream of a VFO of this front end (the demodulator is fused into the channel)"); }
        return v;
    }

    dsp::stream<dsp::complex_t> dummyOut;  // what `out` names until a channel is bound (the one-argument constructor): never written
    IQFrontEnd* fe;
    RxVFO* vfo = nullptr;
};

}  // namespace sdrpp_gpu
