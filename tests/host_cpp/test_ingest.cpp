// Raw wire formats through the C++ host blocks (IQFrontEnd::ingestRaw / ingestServerFrame -> sdrpp_push_raw): a source that drives the front end itself hands
// it the bytes its radio delivered — int8 for the first half of the blocks, uint8 with the rtl_sdr table (sdrpp_design_u8_table) from block `switch_at` on —
// and then the frames of a server connection.  One WFM radio, one consumer bound with bindIQStream; the front end's worker is never started: every block is
// processed and handed out before the call returns.  tests/test_ingest_host_cpp.py pushes the floats numpy makes of the same bytes through the C-ABI: the
// bound consumer's floats and the radio's audio must be exactly those, block by block, nothing lost or doubled.
//   usage: test_ingest <plans.bin> <raw.bin> <frames.bin> <sample_rate> <block> <switch_at> <outdir>
//   raw.bin: blocks of 2 * block bytes; frames.bin: [i32 length][frame bytes] ...
#include <atomic>
#include <chrono>
#include <cstdio>
#include <fstream>
#include <string>
#include <thread>
#include <vector>
#include "../../sdrplusplus_amd/host/sdrpp_gpu_blocks.h"

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
static std::vector<uint8_t> slurp(const char* path) {
    std::ifstream f(path, std::ios::binary | std::ios::ate);
    std::vector<uint8_t> v((size_t)f.tellg());
    f.seekg(0);
    f.read((char*)v.data(), (std::streamsize)v.size());
    return v;
}

int main(int argc, char** argv) {
    if (argc < 8) { fprintf(stderr, "usage\n"); return 2; }
    sdrpp_gpu::DecimPlans plans;
    if (!plans.load(argv[1])) { fprintf(stderr, "cannot load plans\n"); return 1; }
    const std::vector<uint8_t> raw = slurp(argv[2]), frames = slurp(argv[3]);
    const double sr = atof(argv[4]);
    const int block = atoi(argv[5]), switchAt = atoi(argv[6]);
    const std::string outdir = argv[7];
    const int nblocks = (int)(raw.size() / (2 * (size_t)block));

    dsp::stream<dsp::complex_t> src;
    sdrpp_gpu::IQFrontEnd fe;
    fe.init(&src, sr, false, 1, false, 4096, 100.0, sdrpp_gpu::IQFrontEnd::NUTTALL, acquire, release, nullptr, 0, &plans);
    sdrpp_gpu::RxVFO* wfm = fe.addVFO("wfm", 250000.0, 150000.0, 200000.0);
    if (!wfm) { return 1; }
    wfm->attachDemod(sdrpp_gpu::Demod::WFM);
    dsp::stream<dsp::complex_t> tap;
    fe.bindIQStream(&tap);
    std::vector<float> audio, iq;
    std::vector<int> audioCnt, iqCnt;
    std::atomic<int> nA{ 0 }, nI{ 0 };
    std::thread tA(drain<dsp::stereo_t>, &wfm->audio, &audio, &audioCnt, &nA);
    std::thread tI(drain<dsp::complex_t>, &tap, &iq, &iqCnt, &nI);

    float table[256];
    if (sdrpp_design_u8_table(0, 1.0f, table) != SDRPP_OK) { fprintf(stderr, "sdrpp_design_u8_table\n"); return 1; }
    int rc = 0, taken = 0;
    // what the argument rules refuse comes back as -1 and processes nothing
    {
        const sdrpp_iq_format zero{ SDRPP_IQ_I8, 0.0f, nullptr }, noTable{ SDRPP_IQ_U8, 0.0f, nullptr };
        if (fe.ingestRaw(raw.data(), block, zero) >= 0 || fe.ingestRaw(raw.data(), block, noTable) >= 0 || fe.ingestServerFrame(raw.data(), 5) >= 0) {
            fprintf(stderr, "a bad format was accepted\n");
            rc = 1;
        }
    }
    for (int k = 0; k < nblocks && !rc; k++) {
        const sdrpp_iq_format fmt = k < switchAt ? sdrpp_iq_format{ SDRPP_IQ_I8, 128.0f, nullptr } : sdrpp_iq_format{ SDRPP_IQ_U8, 0.0f, table };
        if (fe.ingestRaw(raw.data() + (size_t)k * 2 * (size_t)block, block, fmt) < 0) {
            fprintf(stderr, "ingestRaw failed at block %d\n", k);
            rc = 1;
        }
        taken++;
    }
    int nframes = 0, frameSamples = 0, delivered = taken;
    for (size_t pos = 0; pos + 4 <= frames.size() && !rc;) {
        int32_t len;
        memcpy(&len, &frames[pos], 4);
        pos += 4;
        const int n = fe.ingestServerFrame(&frames[pos], len);
        if (n < 0) {
            fprintf(stderr, "ingestServerFrame failed at frame %d\n", nframes);
            rc = 1;
        }
        pos += (size_t)len;
        nframes++;
        frameSamples += n > 0 ? n : 0;
        delivered += n > 0 ? 1 : 0;
    }
    {   // the sinks take the last hand-over (a block is swapped in before its ingest call returns; reading it is the sink's business)
        const auto t0 = std::chrono::steady_clock::now();
        while ((nA.load() < delivered || nI.load() < delivered) && std::chrono::steady_clock::now() - t0 < std::chrono::milliseconds(3000)) { std::this_thread::sleep_for(std::chrono::milliseconds(1)); }
    }
    wfm->audio.stopReader();
    tap.stopReader();
    tA.join();
    tI.join();
    auto dump = [&](const char* name, const void* p, size_t n) {
        std::ofstream o(outdir + "/" + name, std::ios::binary);
        o.write((const char*)p, (std::streamsize)n);
    };
    dump("iq.f32", iq.data(), iq.size() * 4);
    dump("iq_counts.i32", iqCnt.data(), iqCnt.size() * 4);
    dump("audio.f32", audio.data(), audio.size() * 4);
    dump("audio_counts.i32", audioCnt.data(), audioCnt.size() * 4);
    printf("blocks %d frames %d frame samples %d iq swaps %zu audio swaps %zu\n", taken, nframes, frameSamples, iqCnt.size(), audioCnt.size());
    return rc;
}
