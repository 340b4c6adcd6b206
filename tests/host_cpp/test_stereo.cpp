// The WFM demodulator's stereo decoder through the C++ host blocks (FusedDemodulator<.., WFM>::setStereo -> RxVFO::setStereo -> sdrpp_vfo_set_stereo): one WFM
// radio fed at its IF rate (250 kS/s in, 250 kS/s out, no channel filter, demodulator bandwidth 150 kHz: the fixture's 75 kHz deviation), pipelined or block
// by block.  A source thread hands blocks over, a sink thread reads getOutput().  tests/test_stereo_host_cpp.py compares the frames with the reference's.
//   usage: test_stereo <plans.bin> <iq.f32> <block> <outdir> <pipelined|bypass> [wait_ms]
#include <atomic>
#include <cstdio>
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

static float* acquire(void*) { static std::vector<float> line(4096); return line.data(); }
static void release(void*) {}

template <class T>
static void drain(dsp::stream<T>* st, std::vector<float>* dst, std::vector<int>* counts, std::atomic<int>* nblocks) {
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

int main(int argc, char** argv) {
    if (argc < 6) { fprintf(stderr, "usage\n"); return 2; }
    sdrpp_gpu::DecimPlans plans;
    if (!plans.load(argv[1])) { fprintf(stderr, "cannot load plans\n"); return 1; }
    std::ifstream f(argv[2], std::ios::binary | std::ios::ate);
    const size_t bytes = (size_t)f.tellg();
    f.seekg(0);
    std::vector<float> iq(bytes / 4);
    f.read((char*)iq.data(), (std::streamsize)bytes);
    const int block = atoi(argv[3]);
    const std::string outdir = argv[4];
    const bool pipelined = std::string(argv[5]) == "pipelined";
    const int waitMs = argc > 6 ? atoi(argv[6]) : 20000;
    const int nblocks = (int)(iq.size() / 2 / (size_t)block);

    dsp::stream<dsp::complex_t> src;
    sdrpp_gpu::IQFrontEnd fe;
    fe.init(&src, 250000.0, false, 1, false, 4096, 100.0, sdrpp_gpu::IQFrontEnd::NUTTALL, acquire, release, nullptr, 0, &plans);
    sdrpp_gpu::RxVFO* wfm = fe.addVFO("wfm", 250000.0, 250000.0, 0.0);
    sdrpp_gpu::RxVFO* plain = fe.addVFO("plain", 50000.0, 12500.0, 20000.0);
    if (!wfm || !plain) { return 1; }
    plain->attachDemod(sdrpp_gpu::Demod::NFM);
    {
        bool threw = false;
        try { plain->setStereo(true); } catch (const std::runtime_error&) { threw = true; }  // the decoder belongs to the WFM demodulator
        if (!threw || plain->stereoOn) { fprintf(stderr, "stereo on an NFM radio\n"); return 1; }
    }
    sdrpp_gpu::FusedDemodulator<demod::Demodulator, sdrpp_gpu::Demod::WFM> fused(&fe);
    fused.init("wfm", nullptr, &wfm->out, 150000.0, 48000.0);
    fused.setStereo(true);
    if (!wfm->stereoOn || fused.getOutput() != &wfm->audio) { fprintf(stderr, "setStereo(true)\n"); return 1; }
    if (pipelined) { fe.setPipelining(true, 4); }
    fe.setStopGrace(waitMs);
    std::vector<float> audio, plainAudio;
    std::vector<int> cnt, plainCnt;
    std::atomic<int> nA{ 0 }, nP{ 0 };
    std::thread tA(drain<dsp::stereo_t>, fused.getOutput(), &audio, &cnt, &nA);
    std::thread tP(drain<dsp::stereo_t>, &plain->audio, &plainAudio, &plainCnt, &nP);
    fe.start();
    size_t pos = 0;
    for (int k = 0; k < nblocks; k++) {
        memcpy(src.writeBuf, &iq[2 * pos], sizeof(float) * 2 * (size_t)block);
        if (!src.swap(block)) { fprintf(stderr, "source stream stopped at block %d\n", k); return 1; }
        pos += (size_t)block;
    }
    {
        const auto t0 = std::chrono::steady_clock::now();
        while (fe.blocksTaken() < (uint64_t)nblocks) {
            if (std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(waitMs)) { fprintf(stderr, "the last block was not taken in time\n"); return 1; }
            std::this_thread::sleep_for(std::chrono::microseconds(200));
        }
    }
    fe.stop();
    if (fe.drainPipeline() < 0) { fprintf(stderr, "drainPipeline\n"); return 1; }
    {
        const auto t0 = std::chrono::steady_clock::now();
        while ((nA.load() < nblocks || nP.load() < nblocks) && std::chrono::steady_clock::now() - t0 < std::chrono::milliseconds(3000)) { std::this_thread::sleep_for(std::chrono::milliseconds(1)); }
    }
    wfm->audio.stopReader();
    plain->audio.stopReader();
    tA.join();
    tP.join();
    fused.setStereo(false);
    if (wfm->stereoOn) { fprintf(stderr, "setStereo(false)\n"); return 1; }
    auto dump = [&](const char* name, const void* p, size_t n) {
        std::ofstream o(outdir + "/" + name, std::ios::binary);
        o.write((const char*)p, (std::streamsize)n);
    };
    dump("audio.f32", audio.data(), audio.size() * 4);
    dump("counts.i32", cnt.data(), cnt.size() * 4);
    printf("blocks %d audio %zu frames in %zu swaps, plain %zu blocks\n", nblocks, audio.size() / 2, cnt.size(), plainCnt.size());
    return 0;
}
