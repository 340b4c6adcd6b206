// The radio's IF chain through the C++ control surface while a pipelined graph runs: FusedDemodulator<NFM> with the squelch toggled and its level moved,
// FusedDemodulator<USB> with the noise blanker toggled and its level moved (radio_module.h:633-713 -> sdrpp_gpu_radio.h -> RxVFO::setSquelch /
// setNoiseBlanker -> sdrpp_vfo_set_if).  Same harness as test_reconfig2.cpp: a source thread hands blocks over, sink threads read every stream, the
// setters are called between blocks once the worker has taken the block just handed over:
//     after block 1: NFM squelch on (level stays -100: open)   after block 2: USB blanker on (level 10)     after block 3: NFM squelch level -10 (closes)
//     after block 5: USB blanker level 5                       after block 6: NFM squelch level -40 (opens)  after block 8: USB blanker off
//     after block 9: NFM squelch off
// tests/test_ifchain_host_cpp.py replays the schedule on the oracle with the float32 restatement of the two blocks between RxVFO and demodulator: nothing
// lost, nothing delivered twice, audio equal to a run that had those settings from the matching block on.
//   usage: test_ifchain <plans.bin> <iq.f32> <sample_rate> <block> <outdir> [wait_ms]
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

int main(int argc, char** argv) {
    if (argc < 6) { fprintf(stderr, "usage\n"); return 2; }
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
    const int waitMs = argc > 6 ? atoi(argv[6]) : 20000;
    const int nblocks = (int)(iq.size() / 2 / (size_t)block);

    dsp::stream<dsp::complex_t> src;
    sdrpp_gpu::IQFrontEnd fe;
    fe.init(&src, sr, false, 1, false, 4096, 100.0, sdrpp_gpu::IQFrontEnd::NUTTALL, acquire, release, nullptr, 0, &plans);
    sdrpp_gpu::RxVFO* vNfm = fe.addVFO("nfm", 50000.0, 12500.0, -sr / 4);
    sdrpp_gpu::RxVFO* vUsb = fe.addVFO("usb", 24000.0, 2800.0, sr / 8);
    if (!vNfm || !vUsb) { return 1; }
    sdrpp_gpu::FusedDemodulator<demod::Demodulator, sdrpp_gpu::Demod::NFM> nfm(&fe);
    sdrpp_gpu::FusedDemodulator<demod::Demodulator, sdrpp_gpu::Demod::USB> usb(&fe);
    nfm.init("nfm", nullptr, &vNfm->out, 12500.0, 48000.0);
    usb.init("usb", nullptr, &vUsb->out, 2800.0, 48000.0);
    if (!nfm.getSquelchAllowed() || !usb.getNBAllowed() || nfm.getNBAllowed()) { fprintf(stderr, "allowed flags\n"); return 1; }
    nfm.setSquelchLevel(-250.0f);  // clamped to MIN_SQUELCH
    usb.setNBLevel(99.0f);         // clamped to MAX_NB
    if (vNfm->squelchLevel != -100.0 || vUsb->nbLevel != 10.0 || vNfm->squelchOn || vUsb->nbOn) { fprintf(stderr, "clamps\n"); return 1; }
    fe.setPipelining(true, 4);
    fe.setStopGrace(waitMs);
    std::vector<float> nfmOut, usbOut;
    std::vector<int> nfmCnt, usbCnt;
    std::atomic<int> nfmN{ 0 }, usbN{ 0 };
    std::thread tNfm(drain, nfm.getOutput(), &nfmOut, &nfmCnt, &nfmN);
    std::thread tUsb(drain, usb.getOutput(), &usbOut, &usbCnt, &usbN);
    fe.start();
    auto settled = [&](int k) -> bool {
        const auto t0 = std::chrono::steady_clock::now();
        while (fe.blocksTaken() < (uint64_t)(k + 1)) {
            if (std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(waitMs)) { return false; }
            std::this_thread::sleep_for(std::chrono::microseconds(200));
        }
        return true;
    };
    size_t pos = 0;
    for (int k = 0; k < nblocks; k++) {
        memcpy(src.writeBuf, &iq[2 * pos], sizeof(float) * 2 * (size_t)block);
        if (!src.swap(block)) { fprintf(stderr, "source stream stopped at block %d\n", k); return 1; }
        pos += (size_t)block;
        if (k >= 1 && k <= 9) {
            if (!settled(k)) { fprintf(stderr, "block %d was not taken in time\n", k); return 1; }
        }
        if (k == 1) { nfm.setSquelchEnabled(true); }
        if (k == 2) { usb.setNBEnabled(true); }
        if (k == 3) { nfm.setSquelchLevel(-10.0f); }
        if (k == 5) { usb.setNBLevel(5.0f); }
        if (k == 6) { nfm.setSquelchLevel(-40.0f); }
        if (k == 8) { usb.setNBEnabled(false); }
        if (k == 9) { nfm.setSquelchEnabled(false); }
    }
    if (!settled(nblocks - 1)) { fprintf(stderr, "the last block was not taken in time\n"); return 1; }
    fe.stop();
    if (fe.drainPipeline() < 0) { fprintf(stderr, "drainPipeline\n"); return 1; }
    {
        const auto t0 = std::chrono::steady_clock::now();
        while ((nfmN.load() < nblocks || usbN.load() < nblocks) && std::chrono::steady_clock::now() - t0 < std::chrono::milliseconds(3000)) { std::this_thread::sleep_for(std::chrono::milliseconds(1)); }
        std::this_thread::sleep_for(std::chrono::milliseconds(20));
    }
    nfm.getOutput()->stopReader();
    usb.getOutput()->stopReader();
    tNfm.join();
    tUsb.join();
    auto dump = [&](const char* name, const void* p, size_t n) {
        std::ofstream o(outdir + "/" + name, std::ios::binary);
        o.write((const char*)p, (std::streamsize)n);
    };
    dump("nfm.f32", nfmOut.data(), nfmOut.size() * 4);
    dump("nfm_counts.i32", nfmCnt.data(), nfmCnt.size() * 4);
    dump("usb.f32", usbOut.data(), usbOut.size() * 4);
    dump("usb_counts.i32", usbCnt.data(), usbCnt.size() * 4);
    printf("blocks %d nfm %zu in %zu blocks, usb %zu in %zu\n", nblocks, nfmOut.size() / 2, nfmCnt.size(), usbOut.size() / 2, usbCnt.size());
    return 0;
}
