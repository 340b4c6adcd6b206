// The recorder sink through the C++ host blocks (RxVFO::attachRecorder -> sdrpp_vfo_set_rec; misc_modules/recorder behind a radio's audio stream): a graph
// with two radios, one of them recorded (WFM with the AF chain to 48 kHz, volume 0.9, mono, INT16, "ignore silence" on), run pipelined or block by block.
// A source thread hands blocks over, sink threads read `audio` of both radios and `recorded` of the first; after block 6 the recorded radio is re-planned
// (setOutSamplerate: a new handle on the device — the recorder must stay).  The input holds a stretch of exact zeros, so some blocks are silent.
// tests/test_recorder_host_cpp.py applies the float32 restatement of tests/test_recorder.py to every block `audio` carried: `recorded` must carry exactly
// those bytes, one swap per block that is not silent, and the level getter the running maximum of the blocks' peaks.
//   usage: test_recorder <plans.bin> <iq.f32> <sample_rate> <block> <outdir> <pipelined|bypass> [wait_ms]
#include <atomic>
#include <cstdio>
#include <fstream>
#include <string>
#include <thread>
#include <vector>
#include "../../sdrplusplus_amd/host/sdrpp_gpu_blocks.h"

static float* acquire(void*) { static std::vector<float> line(4096); return line.data(); }
static void release(void*) {}

template <class T, class E>
static void drain(dsp::stream<T>* st, std::vector<E>* dst, std::vector<int>* counts, std::atomic<int>* nblocks) {
    while (true) {
        int n = st->read();
        if (n < 0) { break; }
        const E* p = (const E*)st->readBuf;
        dst->insert(dst->end(), p, p + (sizeof(T) / sizeof(E)) * (size_t)n);
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
    sdrpp_gpu::RxVFO* rec = fe.addVFO("rec", 250000.0, 150000.0, 600000.0);
    sdrpp_gpu::RxVFO* plain = fe.addVFO("plain", 50000.0, 12500.0, -500000.0);
    if (!rec || !plain) { return 1; }
    rec->attachDemod(sdrpp_gpu::Demod::WFM);
    rec->attachAF(48000.0, 50e-6, false);
    plain->attachDemod(sdrpp_gpu::Demod::NFM);
    {
        bool threw = false;
        try { rec->attachRecorder(1.0, false, 2, false); } catch (const std::runtime_error&) { threw = true; }  // INT32 is not offered
        if (!threw || rec->recOn) { fprintf(stderr, "INT32 accepted\n"); return 1; }
    }
    rec->attachRecorder(0.5, false, 3, false);
    rec->attachRecorder(0.9, true, 1, true);  // (a second call only changes the parameters)
    const dsp::stereo_t l0 = rec->getRecorderLevel();
    if (l0.l != 0.0f || l0.r != 0.0f) { fprintf(stderr, "level before the first block\n"); return 1; }
    if (pipelined) { fe.setPipelining(true, 4); }
    fe.setStopGrace(waitMs);
    std::vector<float> recAudio, plainAudio;
    std::vector<uint8_t> recBytes;
    std::vector<int> recAudioCnt, plainCnt, recBytesCnt;
    std::atomic<int> nA{ 0 }, nP{ 0 }, nB{ 0 };
    std::thread tA(drain<dsp::stereo_t, float>, &rec->audio, &recAudio, &recAudioCnt, &nA);
    std::thread tP(drain<dsp::stereo_t, float>, &plain->audio, &plainAudio, &plainCnt, &nP);
    std::thread tB(drain<uint8_t, uint8_t>, &rec->recorded, &recBytes, &recBytesCnt, &nB);
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
        if (k == 6) {
            if (!settled(k)) { fprintf(stderr, "block %d was not taken in time\n", k); return 1; }
            rec->setOutSamplerate(250000.0, 140000.0);  // a re-plan: the VFO gets a new handle, the recorder stays
            if (!rec->recOn) { fprintf(stderr, "recorder lost\n"); return 1; }
        }
    }
    if (!settled(nblocks - 1)) { fprintf(stderr, "the last block was not taken in time\n"); return 1; }
    fe.stop();
    if (pipelined && fe.drainPipeline() < 0) { fprintf(stderr, "drainPipeline\n"); return 1; }
    {
        const auto t0 = std::chrono::steady_clock::now();
        while ((nA.load() < nblocks || nP.load() < nblocks) && std::chrono::steady_clock::now() - t0 < std::chrono::milliseconds(3000)) { std::this_thread::sleep_for(std::chrono::milliseconds(1)); }
        std::this_thread::sleep_for(std::chrono::milliseconds(50));
    }
    rec->audio.stopReader();
    plain->audio.stopReader();
    rec->recorded.stopReader();
    tA.join();
    tP.join();
    tB.join();
    const dsp::stereo_t lvl = rec->getRecorderLevel();
    rec->resetRecorderLevel();
    const dsp::stereo_t lz = rec->getRecorderLevel();
    if (lz.l != 0.0f || lz.r != 0.0f) { fprintf(stderr, "resetRecorderLevel\n"); return 1; }
    auto dump = [&](const char* name, const void* p, size_t n) {
        std::ofstream o(outdir + "/" + name, std::ios::binary);
        o.write((const char*)p, (std::streamsize)n);
    };
    dump("rec_audio.f32", recAudio.data(), recAudio.size() * 4);
    dump("rec_audio_counts.i32", recAudioCnt.data(), recAudioCnt.size() * 4);
    dump("rec_bytes.u8", recBytes.data(), recBytes.size());
    dump("rec_bytes_counts.i32", recBytesCnt.data(), recBytesCnt.size() * 4);
    dump("plain_counts.i32", plainCnt.data(), plainCnt.size() * 4);
    const float level[2] = { lvl.l, lvl.r };
    dump("level.f32", level, sizeof(level));
    printf("blocks %d audio %zu in %zu blocks, recorded %zu bytes in %zu swaps, plain %zu blocks\n", nblocks, recAudio.size() / 2, recAudioCnt.size(), recBytes.size(), recBytesCnt.size(), plainCnt.size());
    return 0;
}
