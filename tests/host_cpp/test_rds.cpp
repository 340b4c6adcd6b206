// The WFM demodulator's RDS branch through the C++ host blocks (RxVFO::attachRDS / setRDSOut -> sdrpp_vfo_set_rds, result flag 32 in a pipelined graph,
// sdrpp_vfo_rds_read block by block; FusedDemodulator<.., WFM>::setRDSOut / getRDSOutput): a graph with a WFM radio that carries the branch and an NFM radio
// without, run pipelined or block by block.  A source thread hands blocks over, sink threads read `audio` of both radios and `rdsOut` of the first.  Behind
// block 3 the front end is stopped and started, behind block 5 pipelining is switched the other way and behind block 6 back, block 8 runs with the branch
// switched off (setRDSOut(false) behind block 7, true behind block 8).  tests/test_rds_host_cpp.py pushes the same blocks through the C-ABI with the same
// switch: `rdsOut` must carry exactly those samples, one swap per block that produced any, nothing lost or doubled.
//   usage: test_rds <plans.bin> <iq.f32> <sample_rate> <block> <outdir> <pipelined|bypass> [wait_ms]
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

    dsp::stream<dsp::complex_t> src;
    sdrpp_gpu::IQFrontEnd fe;
    fe.init(&src, sr, false, 1, false, 4096, 100.0, sdrpp_gpu::IQFrontEnd::NUTTALL, acquire, release, nullptr, 0, &plans);
    sdrpp_gpu::RxVFO* wfm = fe.addVFO("wfm", 250000.0, 150000.0, 200000.0);
    sdrpp_gpu::RxVFO* plain = fe.addVFO("plain", 50000.0, 12500.0, -300000.0);
    if (!wfm || !plain) { return 1; }
    wfm->attachDemod(sdrpp_gpu::Demod::WFM);
    plain->attachDemod(sdrpp_gpu::Demod::NFM);
    {
        bool threw = false;
        try { plain->attachRDS(); } catch (const std::runtime_error&) { threw = true; }  // the branch belongs to the WFM demodulator
        if (!threw || plain->rdsAttached) { fprintf(stderr, "RDS on an NFM radio\n"); return 1; }
    }
    wfm->attachRDS();
    if (!wfm->rdsAttached || !wfm->rdsOn) { fprintf(stderr, "attachRDS\n"); return 1; }
    if (pipelined) { fe.setPipelining(true, 4); }
    fe.setStopGrace(waitMs);
    std::vector<float> wfmAudio, plainAudio, rds;
    std::vector<int> wfmCnt, plainCnt, rdsCnt;
    std::atomic<int> nA{ 0 }, nP{ 0 }, nR{ 0 };
    std::thread tA(drain<dsp::stereo_t>, &wfm->audio, &wfmAudio, &wfmCnt, &nA);
    std::thread tP(drain<dsp::stereo_t>, &plain->audio, &plainAudio, &plainCnt, &nP);
    std::thread tR(drain<dsp::complex_t>, &wfm->rdsOut, &rds, &rdsCnt, &nR);
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
        if (k == 3 || k == 5 || k == 6 || k == 7 || k == 8) {
            if (!settled(k)) { fprintf(stderr, "block %d was not taken in time\n", k); return 1; }
        }
        if (k == 3) {
            fe.stop();
            fe.start();
        }
        if (k == 5) { fe.setPipelining(!pipelined, 4); }
        if (k == 6) { fe.setPipelining(pipelined, 4); }
        if (k == 7) { wfm->setRDSOut(false); }
        if (k == 8) { wfm->setRDSOut(true); }
    }
    if (!settled(nblocks - 1)) { fprintf(stderr, "the last block was not taken in time\n"); return 1; }
    fe.stop();
    if (fe.drainPipeline() < 0) { fprintf(stderr, "drainPipeline\n"); return 1; }
    {
        const auto t0 = std::chrono::steady_clock::now();
        while ((nA.load() < nblocks || nP.load() < nblocks || nR.load() < nblocks - 1) && std::chrono::steady_clock::now() - t0 < std::chrono::milliseconds(3000)) { std::this_thread::sleep_for(std::chrono::milliseconds(1)); }
        std::this_thread::sleep_for(std::chrono::milliseconds(50));
    }
    wfm->audio.stopReader();
    plain->audio.stopReader();
    wfm->rdsOut.stopReader();
    tA.join();
    tP.join();
    tR.join();
    // the radio module's wiring: FusedDemodulator<.., WFM>::getRDSOutput() is the channel's rdsOut, setRDSOut drives the channel's switch
    {
        sdrpp_gpu::FusedDemodulator<demod::Demodulator, sdrpp_gpu::Demod::WFM> fused(&fe);
        fused.init("wfm", nullptr, &wfm->out, 150000.0, 48000.0);
        if (fused.getRDSOutput() != &wfm->rdsOut) { fprintf(stderr, "getRDSOutput\n"); return 1; }
        fused.setRDSOut(false);
        if (wfm->rdsOn) { fprintf(stderr, "setRDSOut(false)\n"); return 1; }
        fused.setRDSOut(true);
        if (!wfm->rdsOn || !wfm->rdsAttached) { fprintf(stderr, "setRDSOut(true)\n"); return 1; }
    }
    auto dump = [&](const char* name, const void* p, size_t n) {
        std::ofstream o(outdir + "/" + name, std::ios::binary);
        o.write((const char*)p, (std::streamsize)n);
    };
    dump("rds.f32", rds.data(), rds.size() * 4);
    dump("rds_counts.i32", rdsCnt.data(), rdsCnt.size() * 4);
    dump("wfm_audio.f32", wfmAudio.data(), wfmAudio.size() * 4);
    dump("wfm_counts.i32", wfmCnt.data(), wfmCnt.size() * 4);
    dump("plain_counts.i32", plainCnt.data(), plainCnt.size() * 4);
    printf("blocks %d rds %zu in %zu swaps, wfm audio %zu blocks, plain %zu blocks\n", nblocks, rds.size() / 2, rdsCnt.size(), wfmCnt.size(), plainCnt.size());
    return 0;
}
