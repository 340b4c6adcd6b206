// RDSDemod-shaped adaptor for the radio module (decoder_modules/radio/src/rds_demod.h:12-102, radio_module.h).
//
// In the reference the radio module owns, behind the WFM demodulator's rdsOut stream, an RDSDemod block with a thread of its own: FastAGC -> Costas<2> -> complex
// band-pass -> Costas<2> -> MM<float> -> BinarySlicer -> DifferentialDecoder, with `out` (one decoded bit per symbol) and `soft` (MM's output, swapped only
// while soft output is enabled).  On the GPU that chain is a block of the channel itself behind its RDS branch (sdrpp_vfo_set_rds_demod, source 0): the object
// the module holds does no signal processing of its own.  init() finds the sdrpp_gpu::RxVFO whose `rdsOut` stream it is handed as `in`, attaches the demodulator
// to it (RxVFO::attachRDSDemod) and `out` / `soft` are that channel's rdsBits / rdsSoft streams, filled by the front end's worker — block by block or, with
// IQFrontEnd::setPipelining, out of every block's result slot (flag 128).  From then on the channel's rdsOut is no longer written: nobody reads it.
//
//   #include <sdrpp_gpu_rds.h>
//   sdrpp_gpu::RDSDemod rdsDemod(&sigpath::iqFrontEnd);
//   rdsDemod.init(wfm.getRDSOutput(), false);                 // radio_module.h: rdsDemod.init(&demod.rdsOut, ...)
//   hs.init(rdsDemod.output(), rdsHandler, this);             // the bits go to rds::Decoder as before
//
// start() / stop() have no counterpart (the front end's cover them); they are kept so that the module's call sequence stays valid.
#pragma once
#include <stdexcept>

#include "sdrpp_gpu_blocks.h"

namespace sdrpp_gpu {

class RDSDemod {
public:
    explicit RDSDemod(IQFrontEnd* frontEnd) : out(dummyOut), soft(dummySoft), fe(frontEnd) {}
    RDSDemod(IQFrontEnd* frontEnd, dsp::stream<dsp::complex_t>* in, bool enableSoft) : RDSDemod(bound(frontEnd, in), frontEnd, enableSoft) {}
    ~RDSDemod() {
        if (vfo && fe && fe->vfoOfRDSStream(&vfo->rdsOut) == vfo) { vfo->detachRDSDemod(); }
    }
    RDSDemod(const RDSDemod&) = delete;
    RDSDemod& operator=(const RDSDemod&) = delete;

    // As the reference's: `in` is the WFM demodulator's rdsOut.  A block whose streams are members cannot re-seat them, so an object built with the one-argument
    // constructor is bound by init() and its streams are reached through output() / softOutput(); the three-argument constructor (the reference's
    // RDSDemod(in, enableSoft)) binds at once and `out` / `soft` ARE the channel's streams.  init() on a bound object moves it (the old channel delivers its
    // rdsOut again) or, on the same channel, starts a fresh demodulator.
    void init(dsp::stream<dsp::complex_t>* in, bool enableSoft) {
        RxVFO* v = bound(fe, in);
        if (vfo && vfo != v) { vfo->detachRDSDemod(); }
        vfo = v;
        vfo->attachRDSDemod(enableSoft);
    }
    void setSoftEnabled(bool enable) {
        if (vfo) { vfo->setRDSDemodSoft(enable); }
    }
    void reset() {
        if (vfo) { vfo->resetRDSDemod(); }
    }
    void start() {}
    void stop() {}
    dsp::stream<uint8_t>* output() { return vfo ? &vfo->rdsBits : nullptr; }
    dsp::stream<float>* softOutput() { return vfo ? &vfo->rdsSoft : nullptr; }
    RxVFO* channel() { return vfo; }

    dsp::stream<uint8_t>& out;
    dsp::stream<float>& soft;

private:
    RDSDemod(RxVFO* v, IQFrontEnd* frontEnd, bool enableSoft) : out(v->rdsBits), soft(v->rdsSoft), fe(frontEnd), vfo(v) { vfo->attachRDSDemod(enableSoft); }
    static RxVFO* bound(IQFrontEnd* frontEnd, dsp::stream<dsp::complex_t>* in) {
        RxVFO* v = frontEnd ? frontEnd->vfoOfRDSStream(in) : nullptr;
        if (!v) { throw std::runtime_error("[sdrpp_gpu::RDSDemod] the input is not the rdsOut stream of a VFO of this front end (the demodulator is fused behind the RDS branch)"); }
        return v;
    }

    dsp::stream<uint8_t> dummyOut;   // what `out` / `soft` name until a channel is bound (the one-argument constructor): never written
    dsp::stream<float> dummySoft;
    IQFrontEnd* fe;
    RxVFO* vfo = nullptr;
};

}  // namespace sdrpp_gpu
