// The Meteor QPSK demodulator through the C++ host blocks (sdrpp_gpu::Meteor -> RxVFO::attachQPSK -> sdrpp_vfo_set_qpsk; result flag 256 in a pipelined graph,
// sdrpp_vfo_qpsk_read block by block): a graph with two 150 kS/s channels without a demodulator and an NFM radio beside them.  Channel A is bound to an adaptor
// from the start (the reference's constructor): its `out` has NO reader and must not be written — nothing may block.  Channel B delivers its `out` to a reader
// until, behind block 9, a second adaptor is bound to it with init(); behind block 10 init() binds it again (a fresh demodulator, OQPSK on).  Behind block 3 the
// front end is stopped and started, behind block 5 pipelining is switched the other way and behind block 6 back, behind block 7 A gets setOQPSK(true), behind
// block 8 A is reset().  tests/test_meteor_host_cpp.py pushes the same blocks through the C-ABI with the same calls: `out` and the packed stream must carry
// exactly those values, one swap per block that started a symbol, nothing lost or doubled; B's `out` exactly its samples up to the bind.
//   usage: test_meteor <plans.bin> <iq.f32> <sample_rate> <block> <outdir> <pipelined|bypass> [wait_ms]
#include <atomic>
#include <cstdio>
#include <fstream>
#include <string>
#include <thread>
#include <vector>
#include "../../sdrplusplus_amd/host/sdrpp_gpu_meteor.h"

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
    sdrpp_gpu::RxVFO* chA = fe.addVFO("meteorA", 150000.0, 150000.0, 150000.0);
    sdrpp_gpu::RxVFO* chB = fe.addVFO("meteorB", 150000.0, 150000.0, -150000.0);
    sdrpp_gpu::RxVFO* plain = fe.addVFO("plain", 50000.0, 12500.0, -20000.0);
    if (!chA || !chB || !plain) { return 1; }
    plain->attachDemod(sdrpp_gpu::Demod::NFM);
    {
        bool threw = false;
        try { sdrpp_gpu::Meteor bad(&fe, &src, 72000.0f, 150000, 33, 0.6f, 0.1f, 0.005f, false, false, 1e-6, 0.01); } catch (const std::runtime_error&) { threw = true; }  // not a VFO's output stream
        if (!threw || chA->qpskAttached) { fprintf(stderr, "Meteor on a foreign stream\n"); return 1; }
        threw = false;
        try { plain->attachQPSK(sdrpp_gpu::RxVFO::QPSKParams{ 72000.0, 150000.0, 33, 0.6, 0.1, 0.005, false, false, 1e-6, 0.01 }); } catch (const std::runtime_error&) { threw = true; }  // needs a channel without a demodulator
        if (!threw || plain->qpskAttached) { fprintf(stderr, "attachQPSK on an NFM radio\n"); return 1; }
    }
    sdrpp_gpu::Meteor dspA(&fe, &chA->out, 72000.0f, 150000, 33, 0.6f, 0.1f, 0.005f, false, false, 1e-6, 0.01);  // the module's call (main.cpp:66)
    sdrpp_gpu::Meteor dspB(&fe);                                                                                   // ... bound later by init()
    if (&dspA.out != &chA->qpskOut || dspA.packedOutput() != &chA->qpskPacked || dspB.output() != nullptr) { fprintf(stderr, "streams\n"); return 1; }
    if (!chA->qpskAttached || chB->qpskAttached) { fprintf(stderr, "attachQPSK\n"); return 1; }
    dspA.start();
    if (pipelined) { fe.setPipelining(true, 4); }
    fe.setStopGrace(waitMs);
    std::vector<float> softA, softB, outB, audioP;
    std::vector<int8_t> packedA, packedB;
    std::vector<int> cntSoftA, cntPackedA, cntSoftB, cntPackedB, cntOutB, cntAP;
    std::atomic<int> nA{ 0 }, nAp{ 0 }, nB{ 0 }, nBp{ 0 }, nOB{ 0 }, nAP{ 0 };
    std::thread t1(drain<dsp::complex_t, float>, &dspA.out, &softA, &cntSoftA, &nA, 2);
    std::thread t2(drain<int8_t, int8_t>, dspA.packedOutput(), &packedA, &cntPackedA, &nAp, 1);
    std::thread t3(drain<dsp::complex_t, float>, &chB->qpskOut, &softB, &cntSoftB, &nB, 2);
    std::thread t4(drain<int8_t, int8_t>, &chB->qpskPacked, &packedB, &cntPackedB, &nBp, 1);
    std::thread t5(drain<dsp::complex_t, float>, &chB->out, &outB, &cntOutB, &nOB, 2);  // (chA->out has no reader: a write to it would block the graph)
    std::thread t6(drain<dsp::stereo_t, float>, &plain->audio, &audioP, &cntAP, &nAP, 2);
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
        if (k == 6) { fe.setPipelining(pipelined, 4); }
        if (k == 7) { dspA.setOQPSK(true); }
        if (k == 8) { dspA.reset(); }
        if (k == 9) { dspB.init(&chB->out, 72000.0f, 150000, 33, 0.6f, 0.1f, 0.005f, false, false, 1e-6, 0.01); }
        if (k == 10) { dspB.init(&chB->out, 72000.0f, 150000, 33, 0.6f, 0.1f, 0.005f, false, true, 1e-6, 0.01); }
    }
    if (!settled(nblocks - 1)) { fprintf(stderr, "the last block was not taken in time\n"); return 1; }
    fe.stop();
    if (fe.drainPipeline() < 0) { fprintf(stderr, "drainPipeline\n"); return 1; }
    {
        const auto t0 = std::chrono::steady_clock::now();
        while ((nA.load() < nblocks || nAp.load() < nblocks || nAP.load() < nblocks || nB.load() < nblocks - 10 || nBp.load() < nblocks - 10) &&
               std::chrono::steady_clock::now() - t0 < std::chrono::milliseconds(3000)) { std::this_thread::sleep_for(std::chrono::milliseconds(1)); }
        std::this_thread::sleep_for(std::chrono::milliseconds(50));
    }
    if (dspB.output() != &chB->qpskOut || dspB.packedOutput() != &chB->qpskPacked || dspB.channel() != chB || !chB->qpskP.oqpsk) { fprintf(stderr, "init() did not bind\n"); return 1; }
    dspA.out.stopReader();
    dspA.packedOutput()->stopReader();
    chB->qpskOut.stopReader();
    chB->qpskPacked.stopReader();
    chB->out.stopReader();
    plain->audio.stopReader();
    t1.join(); t2.join(); t3.join(); t4.join(); t5.join(); t6.join();
    auto dump = [&](const char* name, const void* p, size_t n) {
        std::ofstream o(outdir + "/" + name, std::ios::binary);
        o.write((const char*)p, (std::streamsize)n);
    };
    dump("a_soft.f32", softA.data(), softA.size() * 4);
    dump("a_packed.i8", packedA.data(), packedA.size());
    dump("a_soft_counts.i32", cntSoftA.data(), cntSoftA.size() * 4);
    dump("a_packed_counts.i32", cntPackedA.data(), cntPackedA.size() * 4);
    dump("b_soft.f32", softB.data(), softB.size() * 4);
    dump("b_packed.i8", packedB.data(), packedB.size());
    dump("b_soft_counts.i32", cntSoftB.data(), cntSoftB.size() * 4);
    dump("b_packed_counts.i32", cntPackedB.data(), cntPackedB.size() * 4);
    dump("b_out.f32", outB.data(), outB.size() * 4);
    dump("b_out_counts.i32", cntOutB.data(), cntOutB.size() * 4);
    dump("p_audio_counts.i32", cntAP.data(), cntAP.size() * 4);
    printf("blocks %d a %zu symbols in %zu swaps (packed %zu), b %zu in %zu, b out %zu swaps, audio %zu blocks\n", nblocks, softA.size() / 2, cntSoftA.size(), cntPackedA.size(),
           softB.size() / 2, cntSoftB.size(), cntOutB.size(), cntAP.size());
    return 0;
}
