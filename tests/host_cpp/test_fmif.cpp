// FMIF through the C++ control surface while a pipelined graph runs: RxVFO::setFMIFNR (-> sdrpp_vfo_set_fmnr) on a channel without a demodulator, which
// then delivers the IF chain's output on `out`, beside a twin channel at the same offset that delivers the plain IF.  Same harness as test_ifchain.cpp:
// a source thread hands blocks over, sink threads read both streams, the setter is called between blocks once the worker has taken the block just handed over:
//     after block 1: on, 15 bins      after block 3: 31 bins (the delay line is cleared)      after block 5: off (the block keeps its delay line)
//     after block 7: on, 31 bins (it continues from the delay line as it was left)           after block 9: off
// tests/test_fmif_host_cpp.py replays the schedule on the float64 restatement of tests/test_fmif.py over the twin's stream: nothing lost, nothing
// delivered twice, every sample under the comparison rule of that file.
//   usage: test_fmif <plans.bin> <iq.f32> <sample_rate> <block> <outdir> [wait_ms]
#include <atomic>
#include <cstdio>
#include <fstream>
#include <string>
#include <thread>
#include <vector>
#include "../../sdrplusplus_amd/host/sdrpp_gpu_blocks.h"

static float* acquire(void*) { static std::vector<float> line(4096); return line.data(); }
static void release(void*) {}

static void drain(dsp::stream<dsp::complex_t>* st, std::vector<float>* dst, std::vector<int>* counts, std::atomic<int>* nblocks) {
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
    sdrpp_gpu::RxVFO* vNr = fe.addVFO("nr", 24000.0, 24000.0, sr / 8);
    sdrpp_gpu::RxVFO* vIf = fe.addVFO("if", 24000.0, 24000.0, sr / 8);
    if (!vNr || !vIf) { return 1; }
    if (vNr->fmnrOn || vNr->fmnrBins != 32) { fprintf(stderr, "defaults\n"); return 1; }
    fe.setPipelining(true, 4);
    fe.setStopGrace(waitMs);
    std::vector<float> nrOut, ifOut;
    std::vector<int> nrCnt, ifCnt;
    std::atomic<int> nrN{ 0 }, ifN{ 0 };
    std::thread tNr(drain, &vNr->out, &nrOut, &nrCnt, &nrN);
    std::thread tIf(drain, &vIf->out, &ifOut, &ifCnt, &ifN);
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
        if (k == 1) { vNr->setFMIFNR(true, 15); }
        if (k == 3) { vNr->setFMIFNR(true, 31); }
        if (k == 5) { vNr->setFMIFNR(false, 31); }
        if (k == 7) { vNr->setFMIFNR(true, 31); }
        if (k == 9) { vNr->setFMIFNR(false, 31); }
    }
    if (!settled(nblocks - 1)) { fprintf(stderr, "the last block was not taken in time\n"); return 1; }
    fe.stop();
    if (fe.drainPipeline() < 0) { fprintf(stderr, "drainPipeline\n"); return 1; }
    {
        const auto t0 = std::chrono::steady_clock::now();
        while ((nrN.load() < nblocks || ifN.load() < nblocks) && std::chrono::steady_clock::now() - t0 < std::chrono::milliseconds(3000)) { std::this_thread::sleep_for(std::chrono::milliseconds(1)); }
        std::this_thread::sleep_for(std::chrono::milliseconds(20));
    }
    vNr->out.stopReader();
    vIf->out.stopReader();
    tNr.join();
    tIf.join();
    auto dump = [&](const char* name, const void* p, size_t n) {
        std::ofstream o(outdir + "/" + name, std::ios::binary);
        o.write((const char*)p, (std::streamsize)n);
    };
    dump("nr.f32", nrOut.data(), nrOut.size() * 4);
    dump("nr_counts.i32", nrCnt.data(), nrCnt.size() * 4);
    dump("if.f32", ifOut.data(), ifOut.size() * 4);
    dump("if_counts.i32", ifCnt.data(), ifCnt.size() * 4);
    printf("blocks %d nr %zu in %zu blocks, if %zu in %zu\n", nblocks, nrOut.size() / 2, nrCnt.size(), ifOut.size() / 2, ifCnt.size());
    return 0;
}
