// demod::Demodulator-shaped adaptor for the radio module (decoder_modules/radio/src/demod.h:34-61).
//
// In the reference every demodulator is a chain of dsp blocks with their own threads behind the VFO's output stream
// (radio_module.h:419-563: selectedDemod->init(name, &config, ifChain.out, bw, audioSR); afChain.setInput(selectedDemod->getOutput())).
// On the GPU the demodulator is fused behind its channeliser inside the VFO bank, so the object the radio module holds does no
// signal processing of its own: it finds the sdrpp_gpu::RxVFO whose `out` stream it was handed as `input`, attaches the requested
// demodulator to it (RxVFO::attachDemod) and returns that VFO's `audio` stream from getOutput().  The interface is taken from
// whatever header declares it — `Base` is the radio module's demod::Demodulator inside an SDR++ tree — so this file restates
// nothing but the per-mode constants of demodulators/{wfm,nfm,am,usb,lsb,dsb,cw}.h.
//
//   #include "demod.h"                                   // radio module: declares demod::Demodulator
//   #include <sdrpp_gpu_radio.h>
//   using GpuWFM = sdrpp_gpu::FusedDemodulator<demod::Demodulator, sdrpp_gpu::Demod::WFM>;
//   using GpuCW = sdrpp_gpu::FusedDemodulator<demod::Demodulator, sdrpp_gpu::Demod::CW>;   // setTone / setAGCAttack / setAGCDecay: cw.h's menu
//   ... demod = new GpuWFM(&sigpath::iqFrontEnd);  demod->init(name, &config, vfo->output, bw, audioSR);
//
// The radio module's IF chain (radio_module.h:84-96) sits between the VFO and the demodulator; a fused VFO has no place for CPU blocks
// there, so its three blocks run on the device: the noise blanker and the power squelch (setNBEnabled / setNBLevel /
// setSquelchEnabled / setSquelchLevel below, with the radio module's clamps; sdrpp_vfo_set_if) and, for the FM modes, FMIF, the
// "IF Noise Reduction" (setFMIFNREnabled / setIFNRPreset; sdrpp_vfo_set_fmnr).  The radio module keeps its own `nb` / `powerSquelch` /
// `fmnr` blocks disabled and forwards its menu / interface commands to these setters.
// Not covered: the AF-side CTCSS squelch — with it enabled the demodulator's input is no longer a VFO's own stream and init() /
// setInput() throw, as before.
// showMenu() draws nothing (GUI is out of scope); the options it would toggle are setLowPass / setAGC* / setCarrierAgc below.
#pragma once
#include <stdexcept>
#include <string>

#include "sdrpp_gpu_blocks.h"

class ConfigManager;  // core/src/config.h (only ever passed through)

namespace sdrpp_gpu {

// Per-mode constants of the radio module's analog demodulators (decoder_modules/radio/src/demodulators/*.h, "INFO" blocks:
// wfm.h:267-282, nfm.h:55-70, am.h:75-90, usb.h:69-84, lsb.h:68-83, dsb.h:68-83, cw.h:81-96).  vfoReference: ImGui::WaterfallVFO::REF_LOWER = 0,
// REF_CENTER = 1, REF_UPPER = 2 (gui/widgets/waterfall.h:26-30); deemphasis mode: DEEMP_MODE_50US = 1, DEEMP_MODE_NONE = 3
// (demod.h:8-14).
struct DemodInfo {
    const char* name;
    double ifSampleRate, defaultBandwidth, minBandwidth, maxBandwidth, defaultSnapInterval;
    int vfoReference;
    bool deempAllowed;
    int defaultDeemphasisMode;
    bool fmIfnrAllowed, nbAllowed;
};
inline const DemodInfo& demodInfo(Demod m) {
    static const DemodInfo wfm{ "WFM", 250000.0, 150000.0, 50000.0, 250000.0, 100000.0, 1, true, 1, true, false };
    static const DemodInfo nfm{ "FM", 50000.0, 12500.0, 1000.0, 50000.0, 2500.0, 1, true, 3, true, false };
    static const DemodInfo am{ "AM", 15000.0, 10000.0, 1000.0, 15000.0, 1000.0, 1, false, 3, false, false };
    static const DemodInfo usb{ "USB", 24000.0, 2800.0, 500.0, 12000.0, 100.0, 0, false, 3, false, true };
    static const DemodInfo lsb{ "LSB", 24000.0, 2800.0, 500.0, 12000.0, 100.0, 2, false, 3, false, true };
    static const DemodInfo dsb{ "DSB", 24000.0, 4600.0, 1000.0, 12000.0, 100.0, 1, false, 3, false, true };
    static const DemodInfo cw{ "CW", 3000.0, 200.0, 50.0, 500.0, 10.0, 1, false, 3, false, false };
    switch (m) {
    case Demod::WFM: return wfm;
    case Demod::NFM: return nfm;
    case Demod::AM: return am;
    case Demod::USB: return usb;
    case Demod::LSB: return lsb;
    case Demod::CW: return cw;
    default: return dsb;
    }
}

template <class Base, Demod MODE>
class FusedDemodulator : public Base {
public:
    explicit FusedDemodulator(IQFrontEnd* frontEnd) : fe(frontEnd) {}
    ~FusedDemodulator() override {}

    void init(std::string name, ConfigManager* config, dsp::stream<dsp::complex_t>* input, double bandwidth, double audioSR) override {
        (void)config;  // the options live in the radio module's config; the setters below receive them
        (void)audioSR;
        _name = name;
        _bandwidth = bandwidth;
        bind(input);
    }
    // The VFO bank's worker runs the demodulator; starting / stopping it on its own has no counterpart (the front end's start / stop
    // covers it).  Kept so that the radio module's call sequence (demod.h:38-39, radio_module.h:455-473) stays valid.
    void start() override {}
    void stop() override {}
    void showMenu() override {}
    void setBandwidth(double bandwidth) override {
        _bandwidth = bandwidth;
        if (vfo) { vfo->setDemodBandwidth(bandwidth); }
    }
    void setInput(dsp::stream<dsp::complex_t>* input) override { bind(input); }
    void AFSampRateChanged(double newSR) override { (void)newSR; }
    const char* getName() override { return demodInfo(MODE).name; }
    double getIFSampleRate() override { return demodInfo(MODE).ifSampleRate; }
    double getAFSampleRate() override { return getIFSampleRate(); }
    double getDefaultBandwidth() override { return demodInfo(MODE).defaultBandwidth; }
    double getMinBandwidth() override { return demodInfo(MODE).minBandwidth; }
    double getMaxBandwidth() override { return demodInfo(MODE).maxBandwidth; }
    bool getBandwidthLocked() override { return false; }
    double getDefaultSnapInterval() override { return demodInfo(MODE).defaultSnapInterval; }
    int getVFOReference() override { return demodInfo(MODE).vfoReference; }
    bool getDeempAllowed() override { return demodInfo(MODE).deempAllowed; }
    bool getPostProcEnabled() override { return true; }
    int getDefaultDeemphasisMode() override { return demodInfo(MODE).defaultDeemphasisMode; }
    bool getFMIFNRAllowed() override { return demodInfo(MODE).fmIfnrAllowed; }
    bool getNBAllowed() override { return demodInfo(MODE).nbAllowed; }
    bool getHighPassAllowed() override { return MODE != Demod::CW; }  // cw.h:95-96: the one demodulator that allows neither
    bool getSquelchAllowed() override { return MODE != Demod::CW; }
    dsp::stream<dsp::stereo_t>* getOutput() override { return vfo ? &vfo->audio : nullptr; }

    // what the reference's showMenu() toggles (wfm.h:104-111 / nfm.h:37-43 "Low Pass"; am.h:40-63, usb.h:40-57 AGC attack / decay, carrier AGC)
    void setLowPass(bool enabled) { _lowPass = enabled; apply(); }
    void setAGCAttack(double attack) { _agcAttack = attack; apply(); }
    void setAGCDecay(double decay) { _agcDecay = decay; apply(); }
    void setCarrierAgc(bool enabled) { _carrierAgc = enabled; apply(); }
    // CW only (cw.h:62-70, the menu's clamp to 250 .. 1250 Hz): the beat note — the translation's phase stays continuous, nothing restarts
    void setTone(int tone) {
        if (MODE != Demod::CW) { throw std::runtime_error("[sdrpp_gpu::FusedDemodulator] the tone belongs to the CW demodulator"); }
        _tone = tone < 250 ? 250 : (tone > 1250 ? 1250 : tone);
        if (vfo) { vfo->setCWTone((double)_tone); }
    }
    // the radio module's IF chain on the device (radio_module.h:633-713; clamps :908-911: MIN_NB 1, MAX_NB 10, MIN_SQUELCH -100, MAX_SQUELCH 0)
    void setNBEnabled(bool enabled) { _nbEnabled = enabled; applyIF(); }
    void setNBLevel(float level) { _nbLevel = level < 1.0f ? 1.0f : (level > 10.0f ? 10.0f : level); applyIF(); }
    void setSquelchEnabled(bool enabled) { _squelchEnabled = enabled; applyIF(); }
    void setSquelchLevel(float level) { _squelchLevel = level < -100.0f ? -100.0f : (level > 0.0f ? 0.0f : level); applyIF(); }
    // radio_module.h:676-690: the checkbox and the preset (9 / 15 / 31 / 32 bins); WFM runs 32 bins whatever the preset (:531)
    void setFMIFNREnabled(bool enabled) { _fmnrEnabled = enabled; applyIF(); }
    void setIFNRPreset(int bins) { _fmnrBins = bins; applyIF(); }
    // WFM only (wfm.h:79, 118-126: `rdsDemod.init(&demod.rdsOut, ...)`, demod.setRDSOut(_rds)): the demodulator's RDS branch on the device.  A host writes
    // rdsDemod.init(wfm.getRDSOutput(), 5000.0 / 2375, ...) where the reference passes &demod.rdsOut.  DEVIATION: the reference's setRDSOut also clears the
    // discriminator and the audio filter (one click in the audio); here the audio path is left alone.
    void setRDSOut(bool enabled) {
        if (MODE != Demod::WFM) { throw std::runtime_error("[sdrpp_gpu::FusedDemodulator] RDS output belongs to the WFM demodulator"); }
        _rdsOut = enabled;
        if (vfo) { vfo->setRDSOut(enabled); }
    }
    // WFM only (wfm.h `_stereo`, demod.setStereo(_stereo)): the demodulator's stereo decoder on the device; getOutput() then carries (l, r) frames.  As in the
    // reference every switch makes the demodulator start over (BroadcastFM::setStereo calls reset()).
    void setStereo(bool enabled) {
        if (MODE != Demod::WFM) { throw std::runtime_error("[sdrpp_gpu::FusedDemodulator] the stereo decoder belongs to the WFM demodulator"); }
        _stereo = enabled;
        if (vfo) { vfo->setStereo(enabled); }
    }
    // WFM only: the radio's RDSDemod on the device behind the branch (sdrpp_gpu::RDSDemod in sdrpp_gpu_rds.h is the reference-shaped face: hand it getRDSOutput()).
    // These are the hooks for a module that wants the bits without the adaptor object: getRDSBits() / getRDSSoft() are RDSDemod::out / ::soft.
    void setRDSDemod(bool enabled, bool soft = false) {
        if (MODE != Demod::WFM) { throw std::runtime_error("[sdrpp_gpu::FusedDemodulator] the RDS demodulator belongs to the WFM demodulator"); }
        if (!vfo) { return; }
        if (enabled) { vfo->attachRDSDemod(soft); }
        else { vfo->detachRDSDemod(); }
    }
    dsp::stream<uint8_t>* getRDSBits() { return (MODE == Demod::WFM && vfo) ? &vfo->rdsBits : nullptr; }
    dsp::stream<float>* getRDSSoft() { return (MODE == Demod::WFM && vfo) ? &vfo->rdsSoft : nullptr; }
    dsp::stream<dsp::complex_t>* getRDSOutput() { return (MODE == Demod::WFM && vfo) ? &vfo->rdsOut : nullptr; }
    RxVFO* channel() { return vfo; }

private:
    void bind(dsp::stream<dsp::complex_t>* input) {
        RxVFO* v = fe ? fe->vfoOfStream(input) : nullptr;
        if (!v) {
            throw std::runtime_error("[sdrpp_gpu::FusedDemodulator] the input is not the output stream of a VFO of this front end "
                                     "(noise blanker, squelch and FMIF run on the device — setNBEnabled / setSquelchEnabled / setFMIFNREnabled; the CTCSS squelch must stay disabled: "
                                     "the demodulator is fused behind the channeliser)");
        }
        if (vfo && vfo != v) {  // the previous channel goes back to delivering its IF
            vfo->setNoiseBlanker(false, _nbLevel);
            vfo->setSquelch(false, _squelchLevel);
            vfo->setFMIFNR(false, vfo->fmnrBins);
            if (vfo->rdsAttached) { vfo->detachRDS(); }
            if (vfo->stereoOn) { vfo->setStereo(false); }
            vfo->attachDemod(Demod::RAW);
        }
        vfo = v;
        apply();
        applyIF();
        if (MODE == Demod::WFM && _rdsOut) { vfo->setRDSOut(true); }
        if (MODE == Demod::WFM && _stereo) { vfo->setStereo(true); }
    }
    void apply() {
        if (!vfo) { return; }
        vfo->demodBandwidth = _bandwidth;
        if (MODE == Demod::CW) { vfo->cwTone = (double)_tone; }
        vfo->attachDemod(MODE, _lowPass, _agcAttack, _agcDecay, _carrierAgc);
    }

    void applyIF() {
        if (!vfo) { return; }
        if (vfo->nbOn != _nbEnabled || vfo->nbLevel != (double)_nbLevel) { vfo->setNoiseBlanker(_nbEnabled, _nbLevel); }
        if (vfo->squelchOn != _squelchEnabled || vfo->squelchLevel != (double)_squelchLevel) { vfo->setSquelch(_squelchEnabled, _squelchLevel); }
        const bool fmnr = _fmnrEnabled && getFMIFNRAllowed();
        const int bins = (MODE == Demod::WFM) ? 32 : _fmnrBins;
        if (vfo->fmnrOn != fmnr || vfo->fmnrBins != bins) { vfo->setFMIFNR(fmnr, bins); }
    }

    IQFrontEnd* fe;
    RxVFO* vfo = nullptr;
    std::string _name;
    double _bandwidth = 0.0;
    bool _lowPass = true, _carrierAgc = false;
    double _agcAttack = (MODE == Demod::CW) ? 100.0 : 50.0, _agcDecay = 5.0;  // am.h:98-99, usb.h:92-93; cw.h:105-106
    int _tone = 800;  // cw.h:107
    bool _nbEnabled = false, _squelchEnabled = false, _fmnrEnabled = false;
    bool _rdsOut = false;
    bool _stereo = false;
    int _fmnrBins = 32;  // radio_module.h:91
    float _nbLevel = 10.0f, _squelchLevel = -100.0f;  // radio_module.h:906, :446
};

}  // namespace sdrpp_gpu
