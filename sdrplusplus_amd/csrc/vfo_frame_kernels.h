// The framer behind a symbol branch: 4FSK slicer, sync search at every bit offset, descrambled and de-interleaved frames.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <sdrpp_gfx950.h>

namespace sdrpp_k {

// =====================================================================================================================
// M17Slice4FSK and M17FrameDemux (decoder_modules/m17_decoder/src/m17dsp.h:96-276), per soft symbol `val` of the clock recovery and per bit:
//     bits  = val < 0.0f,  fabsf(val) > high_cut
//     demux over delay[0 .. 16 + count) (the 16 newest bits of the previous call, then this call's): searching, delay[i .. i + 16) against the sync words at
//           every i; in a frame, 16 steps that only advance, then frame[interleave[k]] = delay[i] ^ scramble[k] for k = 0 .. frame_bits - 1; the frame leaves
//           with its last bit and the search resumes behind it
// One kind of the wavefront-job role (vfo_ifchain_kernels.h), WK_SYM_FRAME, one level behind the loop (WK_SYM_LOOP): ONE wavefront per VFO — the work of a
// channel is parallel over bits, the state machine is the wavefront's own and every lane holds it.
// A job walks its block in chunks of SDRPP_FRAME_CHUNK_BITS new bits through the wavefront's share of the role's LDS:
//   A   the chunk's bit stream as 32-bit words, stream bit j in word j / 32 at bit j % 32: the 16 carried bits, then the chunk's — bit (j - 16) % 2 of symbol
//       (j - 16) / 2.  A lane forms a whole word from 16 symbols of its own: 64 lanes, one pass per chunk, no exchange between lanes
//   M   the match mask, a bit per position i of the chunk: the window A[i .. i + 16), taken with a funnel shift of two neighbouring words, equals a sync word
//       (the words are kept bit-reversed: stream order is LSB first here).  SDRPP_FRAME_CHUNK_BITS / 32 = 64 words: a lane forms one from its 32 windows
//   E   the push ends of a launch group in bits (twice the running sum of the loop's per-push symbol counts)
//   F   the frame under construction, a byte per position (no two lanes of a scatter share a byte: interleave is a permutation).  It lies here for the whole
//       job: a frame carried in from the block before is loaded from the persistent state when the job starts, one still open when the job ends is stored there
// then a wave-uniform walk, push end by push end: searching, the next set bit of M at or behind i and inside the push (a lane per word, wave_first, count
// trailing zeros); in a frame, min(steps left in the frame, bits left in the push or chunk) at once, the lanes scatter.  A complete frame is packed 8 positions
// to a byte, four bytes to a lane, and stored as a record.  Per-push frame counts at every push end.
// No floating-point arithmetic but the two comparisons; no atomics; every store to device memory is a vector store.
// =====================================================================================================================
#ifndef SDRPP_WAVE_LDS_FLOATS
#error "a part of vfo_ifchain_kernels.h, the role's header: include that one"
#endif
#define SDRPP_FRAME_CHUNK_BITS 2048                                   // new bits per chunk: 64 words of M, a lane each
#define SDRPP_FRAME_A_WORDS (SDRPP_FRAME_CHUNK_BITS / 32 + 2)         // 16 carried bits in front, and the word a window at the chunk's end reaches into
#define SDRPP_FRAME_M_WORDS (SDRPP_FRAME_CHUNK_BITS / 32)
#define SDRPP_FRAME_E_WORDS 32                                        // SDRPP_GROUP_MAX push ends
#define SDRPP_FRAME_MAX_BITS 1024                                     // frame_bits at most
#define SDRPP_FRAME_MAX_SYNC 4
#define SDRPP_FRAME_STATE_HEAD 4                                      // words of the persistent state in front of the part-built frame
#define SDRPP_FRAME_LDS_FLOATS (SDRPP_FRAME_A_WORDS + SDRPP_FRAME_M_WORDS + SDRPP_FRAME_E_WORDS + SDRPP_FRAME_MAX_BITS / 4)
static_assert(SDRPP_FRAME_M_WORDS == 64, "the search reads the match mask a lane per word");

struct FrameJob {
    const float* soft;           // the loop's soft values of this block, all pushes of a launch group in one piece
    const int* sym_counts;       // ... and its symbols per push
    uint32_t* state;             // persistent (device): [0] the 16 delay bits (bit k: the k-th oldest), [1] in a frame, [2] its type, [3] its step counter, then frame_bits bytes
    uint8_t* recs;               // the block's records, `stride` bytes apart
    int* counts;                 // frames per push
    const uint32_t* table;       // [frame_bits]: interleave[k] in the low half, scramble[k] in bit 16 (one load per bit; shared by every framer of the description)
    float high_cut;
    int n_sync;
    uint32_t sync[SDRPP_FRAME_MAX_SYNC];  // bit-reversed: the word's first (most significant) bit in bit 0
    int frame_bits, stride;
    int npush;
    int sym_cap;                 // symbols the loop's outputs have room for
    int rec_cap;                 // records `recs` has room for (never reached: (16 + 2 * sym_cap) / (16 + frame_bits) + 1; a bound on the stores all the same)
    int pad;
};
static_assert(sizeof(FrameJob) % 8 == 0, "records lie in an array");

// the 16-bit window at stream bit p of A
__device__ __forceinline__ uint32_t frame_window(const uint32_t* A, int p) {
    const uint64_t w = (uint64_t)A[p >> 5] | ((uint64_t)A[(p >> 5) + 1] << 32);
    return (uint32_t)(w >> (p & 31)) & 0xFFFFu;
}
// word `w` of M (positions 32 w .. 32 w + 31) without the positions in front of a and from b on
__device__ __forceinline__ uint32_t frame_mask_word(uint32_t m, int w, int a, int b) {
    const int lo = w * 32;
    if (a > lo) { m = (a - lo >= 32) ? 0u : (m & (~0u << (a - lo))); }
    if (b < lo + 32) { m = (b - lo <= 0) ? 0u : (m & (~0u >> (32 - (b - lo)))); }
    return m;
}
__device__ __forceinline__ void vfo_sym_frame_body(const FrameJob& job, float* smem) {
    const int lane = threadIdx.x & 63, wv = (int)threadIdx.x >> 6;
    uint32_t* A = reinterpret_cast<uint32_t*>(smem + wv * SDRPP_WAVE_LDS_FLOATS);
    uint32_t* M = A + SDRPP_FRAME_A_WORDS;
    int* E = reinterpret_cast<int*>(M + SDRPP_FRAME_M_WORDS);
    uint8_t* F = reinterpret_cast<uint8_t*>(E + SDRPP_FRAME_E_WORDS);
    const int FB = min(max(job.frame_bits, 8), SDRPP_FRAME_MAX_BITS), RAW = FB + 16;
    const int npush = min(max(job.npush, 1), SDRPP_FRAME_E_WORDS);
    // push ends in bits: lane q sums the counts up to its own push
    if (lane < npush) {
        int cum = 0;
        for (int j = 0; j <= lane; j++) { cum += max(global_load_i32(job.sym_counts, j), 0); }
        E[lane] = 2 * min(cum, job.sym_cap);
    }
    uint32_t delay = (uint32_t)wave_uniform((int)global_load_u32(job.state, 0)) & 0xFFFFu;
    int detect = wave_uniform((int)global_load_u32(job.state, 1)) != 0 ? 1 : 0;
    int type = wave_uniform((int)global_load_u32(job.state, 2));
    int outc = min(max(wave_uniform((int)global_load_u32(job.state, 3)), 0), RAW - 1);
    if (detect) {
        for (int w = lane; w < FB / 4; w += 64) { reinterpret_cast<uint32_t*>(F)[w] = global_load_u32(job.state, SDRPP_FRAME_STATE_HEAD + w); }
    }
    wave_sync();
    const int total = wave_uniform(E[npush - 1]);
    int i = 0, q = 0, cnt = 0, nrec = 0;
#pragma unroll 1
    for (int c0 = 0; c0 < total; c0 += SDRPP_FRAME_CHUNK_BITS) {
        const int cb = min(SDRPP_FRAME_CHUNK_BITS, total - c0), nA = 16 + cb;
        // 1. slice: lane l forms word l of A (lanes 0 and 1 the two behind the 64th as well) — 16 symbols of its own, two bits each; nA is even, so a symbol's
        //    two bits lie in one word
        for (int w = lane; w < SDRPP_FRAME_A_WORDS; w += 64) {
            uint32_t word = 0u;
#pragma unroll 2
            for (int b = 0; b < 32; b += 2) {
                const int j = 32 * w + b;
                if (j < 16) { word |= ((delay >> j) & 3u) << b; }
                else if (j < nA) {
                    const float val = global_load_f32(job.soft, (c0 + (j - 16)) >> 1);
                    word |= ((val < 0.0f) ? 1u : 0u) << b;
                    word |= ((fabsf(val) > job.high_cut) ? 2u : 0u) << b;
                }
            }
            A[w] = word;
        }
        wave_sync();
        // 2. the match mask: lane l forms word l of M from words l and l + 1 of A — 32 windows out of one 64-bit value
        {
            uint32_t m = 0u;
            const int p0 = 32 * lane;
            if (p0 < cb) {
                const uint64_t w = (uint64_t)A[lane] | ((uint64_t)A[lane + 1] << 32);
#pragma unroll 1
                for (int k = 0; k < 32; k++) {
                    const uint32_t win = (uint32_t)(w >> k) & 0xFFFFu;
                    bool hit = false;
#pragma unroll
                    for (int s = 0; s < SDRPP_FRAME_MAX_SYNC; s++) { hit = hit || (s < job.n_sync && win == job.sync[s]); }
                    if (hit && p0 + k < cb) { m |= 1u << k; }
                }
            }
            M[lane] = m;
        }
        wave_sync();
        // 3. the walk (every variable of it is the same in every lane)
        const int cend = c0 + cb;
        while (i < cend) {
            while (q < npush - 1 && i >= wave_uniform(E[q])) {
                if (lane == 0) { global_store_u32(job.counts, q, (unsigned)cnt); }
                cnt = 0;
                q++;
            }
            const int pend = (q == npush - 1) ? total : wave_uniform(E[q]);
            const int lim = min(pend, cend);
            if (!detect) {
                const int a = i - c0, b = lim - c0;
                const int L = wave_first(frame_mask_word(M[lane], lane, a, b) != 0u);
                if (L >= 64) {
                    i = lim;
                    continue;
                }
                const int pos = L * 32 + __builtin_ctz(frame_mask_word((uint32_t)wave_uniform((int)M[L]), L, a, b) | 0x80000000u);  // (the guard bit: ctz of 0 is not defined; L's word is not 0)
                const uint32_t win = (uint32_t)wave_uniform((int)frame_window(A, pos));
                type = 0;
#pragma unroll
                for (int s = SDRPP_FRAME_MAX_SYNC - 1; s >= 0; s--) {
                    if (s < job.n_sync && win == job.sync[s]) { type = s; }
                }
                i = c0 + pos;
                detect = 1;
                outc = 0;
                continue;
            }
            const int m = min(RAW - outc, lim - i);
            for (int t = outc + lane; t < outc + m; t += 64) {
                if (t >= 16) {
                    const int k = t - 16, pos = (i - c0) + (t - outc);
                    const uint32_t bit = (A[pos >> 5] >> (pos & 31)) & 1u;
                    const uint32_t tk = global_load_u32(job.table, k);
                    F[tk & 0xFFFFu] = (uint8_t)(bit ^ ((tk >> 16) & 1u));
                }
            }
            outc += m;
            i += m;
            if (outc >= RAW) {
                wave_sync();
                if (nrec < job.rec_cap) {
                    uint8_t* rec = job.recs + (size_t)nrec * (size_t)job.stride;
                    for (int w = lane; w < job.stride / 4; w += 64) {
                        uint32_t word = 0u;
#pragma unroll
                        for (int bb = 0; bb < 4; bb++) {
                            const int r = 4 * w + bb;
                            uint32_t byte = 0u;
                            if (r == 0) { byte = (uint32_t)type; }
                            else if (r >= 2 && (r - 2) < FB / 8) {
                                const uint8_t* f = F + 8 * (r - 2);
#pragma unroll
                                for (int e = 0; e < 8; e++) { byte = (byte << 1) | (uint32_t)(f[e] & 1); }
                            }
                            word |= byte << (8 * bb);
                        }
                        global_store_u32(rec, w, word);
                    }
                    nrec++;
                    cnt++;
                }
                detect = 0;
                outc = 0;
                wave_sync();  // (the next frame's scatter overwrites F)
            }
        }
        // the 16 newest bits go to the next chunk, or to the next block
        delay = (uint32_t)wave_uniform((int)frame_window(A, cb));
        wave_sync();  // (the next chunk overwrites A and M)
    }
    for (; q < npush; q++) {
        if (lane == 0) { global_store_u32(job.counts, q, (unsigned)cnt); }
        cnt = 0;
    }
    if (lane == 0) {
        global_store_u32(job.state, 0, delay);
        global_store_u32(job.state, 1, (unsigned)detect);
        global_store_u32(job.state, 2, (unsigned)type);
        global_store_u32(job.state, 3, (unsigned)outc);
    }
    if (detect) {
        for (int w = lane; w < FB / 4; w += 64) { global_store_u32(job.state, SDRPP_FRAME_STATE_HEAD + w, reinterpret_cast<const uint32_t*>(F)[w]); }
    }
}

// (a call, not inlined, as the other kinds' bodies are: the role's own code and the tick kernel's register allocation stay what they are)
__device__ __attribute__((noinline)) void vfo_sym_frame_call(const FrameJob* j, float* smem) { vfo_sym_frame_body(wave_uniform_job(j), smem); }

}  // namespace sdrpp_k
