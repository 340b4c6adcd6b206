// The pager decoder's DSP through the C++ host blocks (sdrpp_gpu::POCSAGDSP -> RxVFO::attachSymbols -> sdrpp_vfo_set_symbols; result flag 64 in a pipelined graph,
// sdrpp_vfo_sym_read block by block): a graph with two pager channels (2400 baud through the reference's constructor, 1200 baud through init()) and an NFM radio
// without the branch, run pipelined or block by block.  A source thread hands blocks over, sink threads read `out` and `soft` of both decoders and the radio's
// audio.  Behind block 3 the front end is stopped and started, behind block 5 pipelining is switched the other way and behind block 6 back, block 8 runs with the
// first decoder's branch switched off.  tests/test_pager_host_cpp.py pushes the same blocks through the C-ABI with the same switch: `out` and `soft` must carry
// exactly those values, one swap each per block that produced any, nothing lost or doubled.
//   usage: test_pager <plans.bin> <iq.f32> <sample_rate> <block> <outdir> <pipelined|bypass> [wait_ms]
#include <atomic>
#include <cstdio>
#include <fstream>
#include <string>
#include <thread>
#include <vector>
#include "../../sdrplusplus_amd/host/sdrpp_gpu_pager.h"

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
    sdrpp_gpu::RxVFO* chA = fe.addVFO("pagerA", 24000.0, 12500.0, 30000.0);
    sdrpp_gpu::RxVFO* chB = fe.addVFO("pagerB", 24000.0, 12500.0, 30000.0);
    sdrpp_gpu::RxVFO* radio = fe.addVFO("radio", 50000.0, 12500.0, -60000.0);
    if (!chA || !chB || !radio) { return 1; }
    radio->attachDemod(sdrpp_gpu::Demod::NFM);
    {
        bool threw = false;
        try { sdrpp_gpu::POCSAGDSP bad(&fe, &radio->out, 50000.0, 2400.0); } catch (const std::runtime_error&) { threw = true; }  // a channel with a demodulator
        if (!threw || radio->symAttached) { fprintf(stderr, "POCSAGDSP on an NFM radio\n"); return 1; }
        threw = false;
        try { sdrpp_gpu::POCSAGDSP bad(&fe, &src, 24000.0, 2400.0); } catch (const std::runtime_error&) { threw = true; }  // not a VFO's stream
        if (!threw) { fprintf(stderr, "POCSAGDSP on a foreign stream\n"); return 1; }
        threw = false;
        try { sdrpp_gpu::POCSAGDSP bad(&fe, &chA->out, 48000.0, 2400.0); } catch (const std::runtime_error&) { threw = true; }  // another rate than the channel's
        if (!threw || chA->symAttached) { fprintf(stderr, "POCSAGDSP at the wrong rate\n"); return 1; }
    }
    sdrpp_gpu::POCSAGDSP dspA(&fe, &chA->out, 24000.0, 2400.0);  // the reference's POCSAGDSP(in, samplerate, baudrate)
    sdrpp_gpu::POCSAGDSP dspB(&fe);
    dspB.init(&chB->out, 24000.0, 1200.0);                        // ... and its init()
    if (&dspA.out != &chA->symOut || &dspA.soft != &chA->symSoft || dspB.output() != &chB->symOut || dspB.softOutput() != &chB->symSoft) { fprintf(stderr, "streams\n"); return 1; }
    if (!chA->symAttached || !chA->symOn || !chB->symAttached) { fprintf(stderr, "attachSymbols\n"); return 1; }
    dspA.start();
    dspB.start();
    if (pipelined) { fe.setPipelining(true, 4); }
    fe.setStopGrace(waitMs);
    std::vector<uint8_t> bitsA, bitsB;
    std::vector<float> softA, softB, audio;
    std::vector<int> cntBitsA, cntSoftA, cntBitsB, cntSoftB, cntAudio;
    std::atomic<int> nA{ 0 }, nAs{ 0 }, nB{ 0 }, nBs{ 0 }, nR{ 0 };
    std::thread t1(drain<uint8_t, uint8_t>, &dspA.out, &bitsA, &cntBitsA, &nA, 1);
    std::thread t2(drain<float, float>, &dspA.soft, &softA, &cntSoftA, &nAs, 1);
    std::thread t3(drain<uint8_t, uint8_t>, dspB.output(), &bitsB, &cntBitsB, &nB, 1);
    std::thread t4(drain<float, float>, dspB.softOutput(), &softB, &cntSoftB, &nBs, 1);
    std::thread t5(drain<dsp::stereo_t, float>, &radio->audio, &audio, &cntAudio, &nR, 2);
    std::thread t6([&]() { while (chA->out.read() >= 0) { chA->out.flush(); } });  // (the channels' IF streams are delivered as well: somebody reads them)
    std::thread t7([&]() { while (chB->out.read() >= 0) { chB->out.flush(); } });
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
        if (k == 7) { chA->setSymbolsOn(false); }
        if (k == 8) { chA->setSymbolsOn(true); }
    }
    if (!settled(nblocks - 1)) { fprintf(stderr, "the last block was not taken in time\n"); return 1; }
    fe.stop();
    if (fe.drainPipeline() < 0) { fprintf(stderr, "drainPipeline\n"); return 1; }
    {
        const auto t0 = std::chrono::steady_clock::now();
        while ((nA.load() < nblocks - 1 || nAs.load() < nblocks - 1 || nB.load() < nblocks || nBs.load() < nblocks || nR.load() < nblocks) &&
               std::chrono::steady_clock::now() - t0 < std::chrono::milliseconds(3000)) { std::this_thread::sleep_for(std::chrono::milliseconds(1)); }
        std::this_thread::sleep_for(std::chrono::milliseconds(50));
    }
    dspA.out.stopReader();
    dspA.soft.stopReader();
    dspB.output()->stopReader();
    dspB.softOutput()->stopReader();
    radio->audio.stopReader();
    chA->out.stopReader();
    chB->out.stopReader();
    t1.join(); t2.join(); t3.join(); t4.join(); t5.join(); t6.join(); t7.join();
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
    dump("audio.f32", audio.data(), audio.size() * 4);
    dump("audio_counts.i32", cntAudio.data(), cntAudio.size() * 4);
    printf("blocks %d a %zu symbols in %zu swaps, b %zu in %zu, audio %zu blocks\n", nblocks, bitsA.size(), cntBitsA.size(), bitsB.size(), cntBitsB.size(), cntAudio.size());
    return 0;
}
