// The M17 decoder's front through the C++ host blocks (sdrpp_gpu::M17FrameSource -> RxVFO::attachM17 -> sdrpp_vfo_set_symbols + sdrpp_vfo_set_framer; result flags
// 64 and 512 in a pipelined graph, sdrpp_vfo_sym_read / sdrpp_vfo_frame_read block by block): one channel that does nothing to its input (the front end's rate in
// and out, bandwidth = rate, offset 0) with the M17 branch, and an NFM radio beside it, run pipelined or block by block.  A source thread hands blocks over; sink
// threads read the four streams of the frame demux, `diagOut` and the radio's audio.  tests/test_m17_host_cpp.py feeds a case of tests/golden/m17_ref.npz: the
// four streams must carry the reference's recorded frames with the reference's swap counts, the soft symbols its per-block counts.
//   usage: test_m17 <plans.bin> <iq.f32> <sample_rate> <block> <outdir> <pipelined|bypass> [wait_ms]
#include <atomic>
#include <cstdio>
#include <fstream>
#include <string>
#include <thread>
#include <vector>
#include "../../sdrplusplus_amd/host/sdrpp_gpu_m17.h"

static float* acquire(void*) { static std::vector<float> line(4096); return line.data(); }
static void release(void*) {}

template <class T, class E>
static void drain(dsp::stream<T>* st, std::vector<E>* dst, std::vector<int>* counts, std::atomic<int>* nswaps, int per) {
    while (true) {
        int n = st->read();
        if (n < 0) { break; }
        const E* p = (const E*)st->readBuf;
        dst->insert(dst->end(), p, p + (size_t)per * (size_t)n);
        counts->push_back(n);
        st->flush();
        nswaps->fetch_add(1);
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
    sdrpp_gpu::RxVFO* ch = fe.addVFO("m17", sr, sr, 0.0);
    sdrpp_gpu::RxVFO* radio = fe.addVFO("radio", sr, sr / 2, 0.0);
    if (!ch || !radio) { return 1; }
    radio->attachDemod(sdrpp_gpu::Demod::NFM);
    {
        bool threw = false;
        sdrpp_gpu::M17FrameSource bad(&fe);
        try { bad.init(&radio->out, sr); } catch (const std::runtime_error&) { threw = true; }  // a channel with a demodulator
        if (!threw || radio->symAttached) { fprintf(stderr, "M17FrameSource on an NFM radio\n"); return 1; }
        threw = false;
        try { bad.init(&src, sr); } catch (const std::runtime_error&) { threw = true; }  // not a VFO's stream
        if (!threw) { fprintf(stderr, "M17FrameSource on a foreign stream\n"); return 1; }
        threw = false;
        try { bad.init(&ch->out, 2 * sr); } catch (const std::runtime_error&) { threw = true; }  // another rate than the channel's
        if (!threw || ch->symAttached || bad.linkSetupOut()) { fprintf(stderr, "M17FrameSource at the wrong rate\n"); return 1; }
    }
    sdrpp_gpu::M17FrameSource front(&fe);
    front.init(&ch->out, sr);
    if (front.linkSetupOut() != &ch->m17LinkSetup || front.lichOut() != &ch->m17Lich || front.streamOut() != &ch->m17Stream || front.packetOut() != &ch->m17Packet ||
        front.diagOut() != &ch->symSoft || !ch->symAttached || !ch->m17Attached) { fprintf(stderr, "streams\n"); return 1; }
    front.start();
    if (pipelined) { fe.setPipelining(true, 4); }
    fe.setStopGrace(waitMs);
    std::vector<uint8_t> ls, lich, strm, pkt;
    std::vector<float> diag, audio;
    std::vector<int> cLs, cLich, cStrm, cPkt, cDiag, cAudio;
    std::atomic<int> nLs{ 0 }, nLich{ 0 }, nStrm{ 0 }, nPkt{ 0 }, nDiag{ 0 }, nR{ 0 };
    std::thread t1(drain<uint8_t, uint8_t>, front.linkSetupOut(), &ls, &cLs, &nLs, 1);
    std::thread t2(drain<uint8_t, uint8_t>, front.lichOut(), &lich, &cLich, &nLich, 1);
    std::thread t3(drain<uint8_t, uint8_t>, front.streamOut(), &strm, &cStrm, &nStrm, 1);
    std::thread t4(drain<uint8_t, uint8_t>, front.packetOut(), &pkt, &cPkt, &nPkt, 1);
    std::thread t5(drain<float, float>, front.diagOut(), &diag, &cDiag, &nDiag, 1);
    std::thread t6(drain<dsp::stereo_t, float>, &radio->audio, &audio, &cAudio, &nR, 2);
    std::thread t7([&]() { while (ch->out.read() >= 0) { ch->out.flush(); } });  // (the channel's IF stream is delivered as well: somebody reads it)
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
        if (k == 2) {  // stop and start in mid-stream (inside a frame): nothing of the branch or the framer is lost
            if (!settled(k)) { fprintf(stderr, "block %d was not taken in time\n", k); return 1; }
            fe.stop();
            fe.start();
        }
    }
    if (!settled(nblocks - 1)) { fprintf(stderr, "the last block was not taken in time\n"); return 1; }
    fe.stop();
    if (fe.drainPipeline() < 0) { fprintf(stderr, "drainPipeline\n"); return 1; }
    {
        const auto t0 = std::chrono::steady_clock::now();
        while ((nDiag.load() < nblocks || nR.load() < nblocks) && std::chrono::steady_clock::now() - t0 < std::chrono::milliseconds(3000)) { std::this_thread::sleep_for(std::chrono::milliseconds(1)); }
        std::this_thread::sleep_for(std::chrono::milliseconds(50));
    }
    front.linkSetupOut()->stopReader();
    front.lichOut()->stopReader();
    front.streamOut()->stopReader();
    front.packetOut()->stopReader();
    front.diagOut()->stopReader();
    radio->audio.stopReader();
    ch->out.stopReader();
    t1.join(); t2.join(); t3.join(); t4.join(); t5.join(); t6.join(); t7.join();
    auto dump = [&](const char* name, const void* p, size_t n) {
        std::ofstream o(outdir + "/" + name, std::ios::binary);
        o.write((const char*)p, (std::streamsize)n);
    };
    dump("ls.u8", ls.data(), ls.size());
    dump("lich.u8", lich.data(), lich.size());
    dump("stream.u8", strm.data(), strm.size());
    dump("packet.u8", pkt.data(), pkt.size());
    dump("diag.f32", diag.data(), diag.size() * 4);
    dump("ls_counts.i32", cLs.data(), cLs.size() * 4);
    dump("lich_counts.i32", cLich.data(), cLich.size() * 4);
    dump("stream_counts.i32", cStrm.data(), cStrm.size() * 4);
    dump("packet_counts.i32", cPkt.data(), cPkt.size() * 4);
    dump("diag_counts.i32", cDiag.data(), cDiag.size() * 4);
    dump("audio_counts.i32", cAudio.data(), cAudio.size() * 4);
    printf("blocks %d frames: %zu link setup, %zu stream, %zu packet, %zu lich; %zu soft symbols in %zu swaps, audio %zu blocks\n", nblocks, cLs.size(), cStrm.size(), cPkt.size(), cLich.size(),
           diag.size(), cDiag.size(), cAudio.size());
    return 0;
}
