// Signal meters through the C++ host blocks (IQFrontEnd::setSignalMeters -> sdrpp_wf_set_meters; RxVFO::getSignalInfo): a graph with three VFOs, run
// pipelined or block by block, in three phases of six blocks.  The table is changed WHILE blocks are in flight, then the front end is stopped and the
// pipeline drained — so the blocks pushed under the old table are delivered after the new one was set, and their values must still go to the VFOs
// the OLD table names:
//   after block 5:  a.setOffset, b.setBandwidth                (same columns, other bands — from block 6 on)
//   after block 11: removeVFO(b), addVFO(d)                    (columns a, b, c -> a, c, d: a value of column 1 belongs to b before, to c after)
// After each phase the pair every VFO reports is written out; tests/test_meters_host_cpp.py compares them with the C-ABI's own rows for the newest line of
// that phase (an ordinary-pass context over the same samples and tables), bit for bit.
//   usage: test_meters <plans.bin> <iq.f32> <sample_rate> <block> <outdir> <pipelined|bypass> [wait_ms]
#include <atomic>
#include <cstdio>
#include <fstream>
#include <string>
#include <thread>
#include <vector>
#include "../../sdrplusplus_amd/host/sdrpp_gpu_blocks.h"

static float* acquire(void*) { static std::vector<float> line(4096); return line.data(); }
static void release(void*) {}

static void drain(dsp::stream<dsp::complex_t>* st) {
    while (st->read() >= 0) { st->flush(); }
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
    if (nblocks != 18) { fprintf(stderr, "18 blocks expected\n"); return 1; }

    dsp::stream<dsp::complex_t> src;
    sdrpp_gpu::IQFrontEnd fe;
    fe.init(&src, sr, false, 1, false, 4096, 100.0, sdrpp_gpu::IQFrontEnd::NUTTALL, acquire, release, nullptr, 0, &plans);
    sdrpp_gpu::RxVFO* a = fe.addVFO("a", 250000.0, 150000.0, 600000.0);
    sdrpp_gpu::RxVFO* b = fe.addVFO("b", 250000.0, 100000.0, -500000.0);
    sdrpp_gpu::RxVFO* c = fe.addVFO("c", 250000.0, 50000.0, 100000.0);
    sdrpp_gpu::RxVFO* d = nullptr;
    if (!a || !b || !c) { return 1; }
    if (pipelined) { fe.setPipelining(true, 4); }
    fe.setSignalMeters(true);
    fe.setStopGrace(waitMs);
    float s = 0.0f, q = 0.0f;
    if (a->getSignalInfo(s, q) || b->getSignalInfo(s, q) || c->getSignalInfo(s, q)) { fprintf(stderr, "signal info before the first line\n"); return 1; }
    std::thread ta(drain, &a->out), tb(drain, &b->out), tc(drain, &c->out), td;
    std::vector<float> report;  // [phase][a, b, c, d][valid, strength, snr]
    auto note = [&](sdrpp_gpu::RxVFO* v) {
        float st = 0.0f, sn = 0.0f;
        const bool ok = v && v->getSignalInfo(st, sn);
        report.push_back(ok ? 1.0f : 0.0f);
        report.push_back(ok ? st : 0.0f);
        report.push_back(ok ? sn : 0.0f);
    };
    auto settled = [&](int k) -> bool {
        const auto t0 = std::chrono::steady_clock::now();
        while (fe.blocksTaken() < (uint64_t)(k + 1)) {
            if (std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(waitMs)) { return false; }
            std::this_thread::sleep_for(std::chrono::microseconds(200));
        }
        return true;
    };
    size_t pos = 0;
    for (int phase = 0; phase < 3; phase++) {
        fe.start();
        for (int k = phase * 6; k < phase * 6 + 6; k++) {
            memcpy(src.writeBuf, &iq[2 * pos], sizeof(float) * 2 * (size_t)block);
            if (!src.swap(block)) { fprintf(stderr, "source stream stopped at block %d\n", k); return 1; }
            pos += (size_t)block;
        }
        if (!settled(phase * 6 + 5)) { fprintf(stderr, "phase %d: the blocks were not taken in time\n", phase); return 1; }
        // the change, with the worker running and (pipelined) the last blocks' results still on their way
        if (phase == 0) {
            a->setOffset(650000.0);
            b->setBandwidth(80000.0);
        }
        if (phase == 1) {
            b->out.stopReader();
            tb.join();
            fe.removeVFO("b");
            b = nullptr;
            d = fe.addVFO("d", 250000.0, 120000.0, -300000.0);
            if (!d) { return 1; }
            td = std::thread(drain, &d->out);
        }
        fe.stop();
        if (pipelined && fe.drainPipeline() < 0) { fprintf(stderr, "drainPipeline\n"); return 1; }
        note(a);
        note(b);
        note(c);
        note(d);
    }
    a->out.stopReader();
    c->out.stopReader();
    d->out.stopReader();
    ta.join();
    tc.join();
    td.join();
    std::ofstream o(outdir + "/signal.f32", std::ios::binary);
    o.write((const char*)report.data(), (std::streamsize)(report.size() * 4));
    printf("blocks %d phases 3\n", nblocks);
    return 0;
}
