// The radio's RDS demodulator through the C++ host blocks (sdrpp_gpu::RDSDemod -> RxVFO::attachRDSDemod -> sdrpp_vfo_set_rds_demod; result flag 128 in a pipelined
// graph, sdrpp_vfo_rds_demod_read block by block): a graph with two WFM radios that carry the RDS branch.  Radio A's branch is bound to an adaptor from the start
// (the reference's constructor, soft output on): its rdsOut has NO reader and must not be written — nothing may block.  Radio B delivers its rdsOut to a reader
// until, behind block 9, a second adaptor is bound to it with init() (soft off); behind block 10 init() binds it again (a fresh demodulator, soft on).  Behind
// block 3 the front end is stopped and started, behind block 5 pipelining is switched the other way and behind block 6 back, blocks 7 runs with A's soft output
// disabled (setSoftEnabled), behind block 8 A is reset().  tests/test_rds_demod_host_cpp.py pushes the same blocks through the C-ABI with the same calls: `out`
// and `soft` must carry exactly those values, one swap per block that started a symbol, nothing lost or doubled; B's rdsOut exactly its samples up to the bind.
//   usage: test_rds_demod <plans.bin> <iq.f32> <sample_rate> <block> <outdir> <pipelined|bypass> [wait_ms]
#include <atomic>
#include <cstdio>
#include <fstream>
#include <string>
#include <thread>
#include <vector>
#include "../../sdrplusplus_amd/host/sdrpp_gpu_rds.h"

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

template <class T, class E>
static void drain(dsp::stream<T>* st, std::vector<E>* dst, std::vector<int>* counts, std::atomic<int>* nblocks, int per) {
    while (true) {
        int n = st->read();
        if (n < 0) { break; }
        const E* p = (const E*)st->readBuf;
        dst->insert(dst->end(), p, p + (size_t)per * (size_t)n);
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
    sdrpp_gpu::RxVFO* chA = fe.addVFO("wfmA", 250000.0, 150000.0, 200000.0);
    sdrpp_gpu::RxVFO* chB = fe.addVFO("wfmB", 250000.0, 150000.0, -250000.0);
    sdrpp_gpu::RxVFO* plain = fe.addVFO("plain", 50000.0, 12500.0, -20000.0);
    if (!chA || !chB || !plain) { return 1; }
    chA->attachDemod(sdrpp_gpu::Demod::WFM);
    chB->attachDemod(sdrpp_gpu::Demod::WFM);
    plain->attachDemod(sdrpp_gpu::Demod::NFM);
    chA->attachRDS();
    chB->attachRDS();
    {
        bool threw = false;
        try { sdrpp_gpu::RDSDemod bad(&fe, &chA->out, false); } catch (const std::runtime_error&) { threw = true; }  // not an rdsOut stream
        if (!threw || chA->rdsdAttached) { fprintf(stderr, "RDSDemod on a foreign stream\n"); return 1; }
        threw = false;
        try { plain->attachRDSDemod(false); } catch (const std::runtime_error&) { threw = true; }  // the demodulator belongs behind a WFM radio's branch
        if (!threw || plain->rdsdAttached) { fprintf(stderr, "attachRDSDemod on an NFM radio\n"); return 1; }
    }
    sdrpp_gpu::RDSDemod dspA(&fe, &chA->rdsOut, true);  // the reference's RDSDemod(in, enableSoft)
    sdrpp_gpu::RDSDemod dspB(&fe);                       // ... bound later by init()
    if (&dspA.out != &chA->rdsBits || &dspA.soft != &chA->rdsSoft || dspB.output() != nullptr) { fprintf(stderr, "streams\n"); return 1; }
    if (!chA->rdsdAttached || !chA->rdsdSoft || chB->rdsdAttached) { fprintf(stderr, "attachRDSDemod\n"); return 1; }
    dspA.start();
    if (pipelined) { fe.setPipelining(true, 4); }
    fe.setStopGrace(waitMs);
    std::vector<uint8_t> bitsA, bitsB;
    std::vector<float> softA, softB, audioA, audioB, audioP, rdsB;
    std::vector<int> cntBitsA, cntSoftA, cntBitsB, cntSoftB, cntAA, cntAB, cntAP, cntRdsB;
    std::atomic<int> nA{ 0 }, nAs{ 0 }, nB{ 0 }, nBs{ 0 }, nAA{ 0 }, nAB{ 0 }, nAP{ 0 }, nRB{ 0 };
    std::thread t1(drain<uint8_t, uint8_t>, &dspA.out, &bitsA, &cntBitsA, &nA, 1);
    std::thread t2(drain<float, float>, &dspA.soft, &softA, &cntSoftA, &nAs, 1);
    std::thread t3(drain<uint8_t, uint8_t>, &chB->rdsBits, &bitsB, &cntBitsB, &nB, 1);
    std::thread t4(drain<float, float>, &chB->rdsSoft, &softB, &cntSoftB, &nBs, 1);
    std::thread t5(drain<dsp::stereo_t, float>, &chA->audio, &audioA, &cntAA, &nAA, 2);
    std::thread t6(drain<dsp::stereo_t, float>, &chB->audio, &audioB, &cntAB, &nAB, 2);
    std::thread t7(drain<dsp::stereo_t, float>, &plain->audio, &audioP, &cntAP, &nAP, 2);
    std::thread t8(drain<dsp::complex_t, float>, &chB->rdsOut, &rdsB, &cntRdsB, &nRB, 2);  // (chA->rdsOut has no reader: a write to it would block the graph)
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
        if (k == 3 || (k >= 5 && k <= 10)) {
            if (!settled(k)) { fprintf(stderr, "block %d was not taken in time\n", k); return 1; }
        }
        if (k == 3) {
            fe.stop();
            fe.start();
        }
        if (k == 5) { fe.setPipelining(!pipelined, 4); }
        if (k == 6) { fe.setPipelining(pipelined, 4); dspA.setSoftEnabled(false); }
        if (k == 7) { dspA.setSoftEnabled(true); }
        if (k == 8) { dspA.reset(); }
        if (k == 9) { dspB.init(&chB->rdsOut, false); }
        if (k == 10) { dspB.init(&chB->rdsOut, true); }
    }
    if (!settled(nblocks - 1)) { fprintf(stderr, "the last block was not taken in time\n"); return 1; }
    fe.stop();
    if (fe.drainPipeline() < 0) { fprintf(stderr, "drainPipeline\n"); return 1; }
    {
        const auto t0 = std::chrono::steady_clock::now();
        while ((nA.load() < nblocks || nAA.load() < nblocks || nAB.load() < nblocks || nAP.load() < nblocks || nB.load() < nblocks - 10) &&
               std::chrono::steady_clock::now() - t0 < std::chrono::milliseconds(3000)) { std::this_thread::sleep_for(std::chrono::milliseconds(1)); }
        std::this_thread::sleep_for(std::chrono::milliseconds(50));
    }
    if (dspB.output() != &chB->rdsBits || dspB.softOutput() != &chB->rdsSoft || dspB.channel() != chB) { fprintf(stderr, "init() did not bind\n"); return 1; }
    dspA.out.stopReader();
    dspA.soft.stopReader();
    chB->rdsBits.stopReader();
    chB->rdsSoft.stopReader();
    chA->audio.stopReader();
    chB->audio.stopReader();
    plain->audio.stopReader();
    chB->rdsOut.stopReader();
    t1.join(); t2.join(); t3.join(); t4.join(); t5.join(); t6.join(); t7.join(); t8.join();
    // the radio module's wiring: FusedDemodulator<.., WFM> hands out the same streams and drives the same switch (the graph is stopped: no delivery runs)
    {
        sdrpp_gpu::FusedDemodulator<demod::Demodulator, sdrpp_gpu::Demod::WFM> fused(&fe);
        fused.init("wfmB", nullptr, &chB->out, 150000.0, 48000.0);
        if (fused.getRDSBits() != &chB->rdsBits || fused.getRDSSoft() != &chB->rdsSoft || fused.getRDSOutput() != &chB->rdsOut) { fprintf(stderr, "getRDSBits\n"); return 1; }
        fused.setRDSDemod(false);
        if (chB->rdsdAttached || !chB->rdsAttached) { fprintf(stderr, "setRDSDemod(false)\n"); return 1; }
        fused.setRDSDemod(true, true);
        if (!chB->rdsdAttached || !chB->rdsdSoft) { fprintf(stderr, "setRDSDemod(true)\n"); return 1; }
        chB->detachRDS();  // the demodulator goes with the branch
        if (chB->rdsdAttached || chB->rdsAttached) { fprintf(stderr, "detachRDS\n"); return 1; }
    }
    auto dump = [&](const char* name, const void* p, size_t n) {
        std::ofstream o(outdir + "/" + name, std::ios::binary);
        o.write((const char*)p, (std::streamsize)n);
    };
    dump("a_bits.u8", bitsA.data(), bitsA.size());
    dump("a_soft.f32", softA.data(), softA.size() * 4);
    dump("a_bits_counts.i32", cntBitsA.data(), cntBitsA.size() * 4);
    dump("a_soft_counts.i32", cntSoftA.data(), cntSoftA.size() * 4);
    dump("b_bits.u8", bitsB.data(), bitsB.size());
    dump("b_soft.f32", softB.data(), softB.size() * 4);
    dump("b_bits_counts.i32", cntBitsB.data(), cntBitsB.size() * 4);
    dump("b_soft_counts.i32", cntSoftB.data(), cntSoftB.size() * 4);
    dump("b_rds.f32", rdsB.data(), rdsB.size() * 4);
    dump("b_rds_counts.i32", cntRdsB.data(), cntRdsB.size() * 4);
    dump("a_audio.f32", audioA.data(), audioA.size() * 4);
    dump("a_audio_counts.i32", cntAA.data(), cntAA.size() * 4);
    dump("b_audio_counts.i32", cntAB.data(), cntAB.size() * 4);
    dump("p_audio_counts.i32", cntAP.data(), cntAP.size() * 4);
    printf("blocks %d a %zu symbols in %zu swaps (soft %zu), b %zu in %zu, b rdsOut %zu swaps, audio %zu / %zu / %zu blocks\n", nblocks, bitsA.size(), cntBitsA.size(), cntSoftA.size(),
           bitsB.size(), cntBitsB.size(), cntRdsB.size(), cntAA.size(), cntAB.size(), cntAP.size());
    return 0;
}
