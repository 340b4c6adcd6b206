// The radio's CW mode through the C++ host blocks (FusedDemodulator<.., CW>: setTone with the menu's clamp, setBandwidth that leaves the tone alone, CW's
// own AGC defaults and INFO block; RxVFO::setCWTone -> sdrpp_vfo_set_ssb_phase_delta): one channel of a running front end goes through the radio module's
// mode switch WFM -> CW -> USB (radio_module.h:419-563: the old demodulator is deleted, the new one initialised on the VFO's stream, then the VFO is told its
// new rate) while a source thread hands blocks over and a sink thread reads `audio`.  Behind block 2 the switch to CW, behind block 4 setTone(600), behind
// block 6 the bandwidth goes to CW's minimum of 50 Hz (a channel filter of 4 560 taps), behind block 8 pipelining is switched the other way and behind
// block 9 back, behind block 10 the switch to USB.  tests/test_cw_host_cpp.py replays the same schedule through the C-ABI: `audio` must carry exactly those
// samples, one swap per producing block, nothing lost or doubled.
//   usage: test_cw <plans.bin> <iq.f32> <sample_rate> <block> <outdir> <pipelined|bypass> [wait_ms]
#include <atomic>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <string>
#include <thread>
#include <vector>
#include "../../sdrplusplus_amd/host/sdrpp_gpu_blocks.h"

// the shape of the radio module's demodulator interface, as far as the adaptor overrides it (a stand-in of this test: inside an SDR++ tree `Base` is
// the radio module's own demod::Demodulator)
class ConfigManager;
namespace demod {
class Demodulator {
public:
    virtual ~Demodulator() {}
    virtual void init(std::string name, ConfigManager* config, dsp::stream<dsp::complex_t>* input, double bandwidth, double audioSR) = 0;
    virtual void start() = 0;
    virtual void stop() = 0;
    virtual void showMenu() = 0;
    virtual void setBandwidth(double bandwidth) = 0;
    virtual void setInput(dsp::stream<dsp::complex_t>* input) = 0;
    virtual void AFSampRateChanged(double newSR) = 0;
    virtual const char* getName() = 0;
    virtual double getIFSampleRate() = 0;
    virtual double getAFSampleRate() = 0;
    virtual double getDefaultBandwidth() = 0;
    virtual double getMinBandwidth() = 0;
    virtual double getMaxBandwidth() = 0;
    virtual bool getBandwidthLocked() = 0;
    virtual double getDefaultSnapInterval() = 0;
    virtual int getVFOReference() = 0;
    virtual bool getDeempAllowed() = 0;
    virtual bool getPostProcEnabled() = 0;
    virtual int getDefaultDeemphasisMode() = 0;
    virtual bool getFMIFNRAllowed() = 0;
    virtual bool getNBAllowed() = 0;
    virtual bool getHighPassAllowed() = 0;
    virtual bool getSquelchAllowed() = 0;
    virtual dsp::stream<dsp::stereo_t>* getOutput() = 0;
};
}  // namespace demod
#include "../../sdrplusplus_amd/host/sdrpp_gpu_radio.h"

using GpuWFM = sdrpp_gpu::FusedDemodulator<demod::Demodulator, sdrpp_gpu::Demod::WFM>;
using GpuCW = sdrpp_gpu::FusedDemodulator<demod::Demodulator, sdrpp_gpu::Demod::CW>;
using GpuUSB = sdrpp_gpu::FusedDemodulator<demod::Demodulator, sdrpp_gpu::Demod::USB>;

static float* acquire(void*) { static std::vector<float> line(4096); return line.data(); }
static void release(void*) {}

static void drain(dsp::stream<dsp::stereo_t>* st, std::vector<float>* dst, std::vector<int>* counts, std::atomic<int>* nblocks) {
    while (true) {
        int n = st->read();
        if (n < 0) { break; }
        const float* p = (const float*)st->readBuf;
        dst->insert(dst->end(), p, p + 2 * (size_t)n);
        counts->push_back(n);
        st->flush();
        nblocks->fetch_add(1);
    }
}

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "check failed: %s (line %d)\n", #cond, __LINE__); return 1; } } while (0)

int main(int argc, char** argv) {
    if (argc < 7) { fprintf(stderr, "usage\n"); return 2; }
    sdrpp_gpu::DecimPlans plans;
    if (!plans.load(argv[1])) { fprintf(stderr, "cannot load plans\n"); return 1; }
    std::ifstream f(argv[2], std::ios::binary | std::ios::ate);
    const size_t bytes = (size_t)f.tellg();
    f.seekg(0);
    std::vector<float> iq(bytes / 4);
    f.read((char*)iq.data(), (std::streamsize)bytes);
    const double sr = atof(argv[3]);
    const int block = atoi(argv[4]);
    const std::string outdir = argv[5];
    const bool pipelined = std::string(argv[6]) == "pipelined";
    const int waitMs = argc > 7 ? atoi(argv[7]) : 20000;
    const int nblocks = (int)(iq.size() / 2 / (size_t)block);

    {   // CW's INFO block (demodulators/cw.h:81-96)
        const sdrpp_gpu::DemodInfo& i = sdrpp_gpu::demodInfo(sdrpp_gpu::Demod::CW);
        CHECK(std::string(i.name) == "CW" && i.ifSampleRate == 3000.0 && i.defaultBandwidth == 200.0 && i.minBandwidth == 50.0 && i.maxBandwidth == 500.0);
        CHECK(i.defaultSnapInterval == 10.0 && i.vfoReference == 1 && !i.deempAllowed && i.defaultDeemphasisMode == 3 && !i.fmIfnrAllowed && !i.nbAllowed);
        CHECK(std::string(sdrpp_gpu::demodInfo(sdrpp_gpu::Demod::DSB).name) == "DSB" && std::string(sdrpp_gpu::demodInfo(sdrpp_gpu::Demod::USB).name) == "USB");
    }
    dsp::stream<dsp::complex_t> src;
    sdrpp_gpu::IQFrontEnd fe;
    fe.init(&src, sr, false, 1, false, 4096, 100.0, sdrpp_gpu::IQFrontEnd::NUTTALL, acquire, release, nullptr, 0, &plans);
    sdrpp_gpu::RxVFO* vfo = fe.addVFO("radio", 250000.0, 150000.0, 200000.0);
    if (!vfo) { return 1; }
    demod::Demodulator* sel = nullptr;
    {
        GpuWFM* w = new GpuWFM(&fe);
        w->init("radio", nullptr, &vfo->out, 150000.0, 48000.0);
        CHECK(w->getHighPassAllowed() && w->getSquelchAllowed());  // every other mode keeps what it returned
        sel = w;
    }
    if (pipelined) { fe.setPipelining(true, 4); }
    fe.setStopGrace(waitMs);
    std::vector<float> audio;
    std::vector<int> cnt;
    std::atomic<int> nA{ 0 };
    std::thread tA(drain, &vfo->audio, &audio, &cnt, &nA);
    fe.start();
    auto settled = [&](int k) -> bool {
        const auto t0 = std::chrono::steady_clock::now();
        while (fe.blocksTaken() < (uint64_t)(k + 1)) {
            if (std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(waitMs)) { return false; }
            std::this_thread::sleep_for(std::chrono::microseconds(200));
        }
        return true;
    };
    GpuCW* cw = nullptr;
    size_t pos = 0;
    for (int k = 0; k < nblocks; k++) {
        memcpy(src.writeBuf, &iq[2 * pos], sizeof(float) * 2 * (size_t)block);
        if (!src.swap(block)) { fprintf(stderr, "source stream stopped at block %d\n", k); return 1; }
        pos += (size_t)block;
        if (k == 2 || k == 4 || k == 6 || k == 8 || k == 9 || k == 10) {
            if (!settled(k)) { fprintf(stderr, "block %d was not taken in time\n", k); return 1; }
        }
        if (k == 2) {  // selectDemod: the old demodulator goes, the new one takes the VFO's stream, then the VFO learns the new IF rate and bandwidth
            delete sel;
            cw = new GpuCW(&fe);
            sel = cw;
            cw->init("radio", nullptr, &vfo->out, cw->getDefaultBandwidth(), 48000.0);
            CHECK(vfo->demod == sdrpp_gpu::Demod::CW && vfo->agcAttack == 100.0 && vfo->agcDecay == 5.0 && vfo->cwTone == 800.0);
            CHECK(!cw->getHighPassAllowed() && !cw->getSquelchAllowed() && cw->getIFSampleRate() == 3000.0 && cw->getOutput() == &vfo->audio);
            vfo->setOutSamplerate(cw->getIFSampleRate(), cw->getDefaultBandwidth());
        }
        if (k == 4) {
            cw->setTone(100);  // the menu's clamp (cw.h:64-66)
            CHECK(vfo->cwTone == 250.0);
            cw->setTone(5000);
            CHECK(vfo->cwTone == 1250.0);
            cw->setTone(600);
            CHECK(vfo->cwTone == 600.0);
        }
        if (k == 6) {  // the radio module's bandwidth change: the VFO's channel filter and the demodulator's own setBandwidth — CW's is empty (cw.h:73)
            vfo->setBandwidth(cw->getMinBandwidth());
            cw->setBandwidth(cw->getMinBandwidth());
            CHECK(vfo->cwTone == 600.0 && vfo->demod == sdrpp_gpu::Demod::CW && vfo->bandwidth == 50.0);  // the tone stays (a re-plan would show in the audio: the AGC would start over)
        }
        if (k == 8) { fe.setPipelining(!pipelined, 4); }
        if (k == 9) { fe.setPipelining(pipelined, 4); }
        if (k == 10) {
            delete sel;
            cw = nullptr;
            GpuUSB* u = new GpuUSB(&fe);
            sel = u;
            u->init("radio", nullptr, &vfo->out, u->getDefaultBandwidth(), 48000.0);
            CHECK(u->getHighPassAllowed() && u->getSquelchAllowed() && vfo->agcAttack == 50.0);
            bool threw = false;
            try { u->setTone(700); } catch (const std::runtime_error&) { threw = true; }  // the tone belongs to CW
            CHECK(threw);
            vfo->setOutSamplerate(u->getIFSampleRate(), u->getDefaultBandwidth());
        }
    }
    if (!settled(nblocks - 1)) { fprintf(stderr, "the last block was not taken in time\n"); return 1; }
    fe.stop();
    if (fe.drainPipeline() < 0) { fprintf(stderr, "drainPipeline\n"); return 1; }
    {
        const auto t0 = std::chrono::steady_clock::now();
        while (nA.load() < nblocks && std::chrono::steady_clock::now() - t0 < std::chrono::milliseconds(3000)) { std::this_thread::sleep_for(std::chrono::milliseconds(1)); }
        std::this_thread::sleep_for(std::chrono::milliseconds(50));
    }
    vfo->audio.stopReader();
    tA.join();
    delete sel;
    auto dump = [&](const char* name, const void* p, size_t n) {
        std::ofstream o(outdir + "/" + name, std::ios::binary);
        o.write((const char*)p, (std::streamsize)n);
    };
    dump("audio.f32", audio.data(), audio.size() * 4);
    dump("counts.i32", cnt.data(), cnt.size() * 4);
    printf("blocks %d audio %zu in %zu swaps\n", nblocks, audio.size() / 2, cnt.size());
    return 0;
}
