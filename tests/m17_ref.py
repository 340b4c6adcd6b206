"""This project's own restatement of the M17 decoder's slicer and frame demultiplexer (M17Slice4FSK, M17FrameDemux: decoder_modules/m17_decoder/src/m17dsp.h),
call by call, for the tests of the framer (sdrpp_vfo_set_framer).  tests/test_m17.py pins it to the fixture recorded from the compiled reference."""
import numpy as np

SEQ = bytes.fromhex("D6B5E23082FF8462BA4E9690D898DD5D0CC85243911DF86E682F35DA14EACD76198DD580D133871357182D2978C3")  # M17 specification: decorrelator sequence
SCRAMBLE = np.unpackbits(np.frombuffer(SEQ, np.uint8)).astype(np.uint8)
INTERLEAVE = np.array([(45 * k + 92 * k * k) % 368 for k in range(368)], np.uint16)                                    # ... its quadratic interleaver
SYNC = (0x55F7, 0xFF5D, 0x75FF)                                                                                      # link setup, stream, packet
HIGH_CUT = (np.float32(1.0) + np.float32(1.0) / np.float32(3.0)) / np.float32(2.0)


def slice4fsk(soft, high_cut=HIGH_CUT):
    """two bits per soft symbol: val < 0, |val| > high_cut (both strict: a NaN gives 0, 0)"""
    soft = np.asarray(soft, np.float32)
    out = np.zeros(2 * len(soft), np.uint8)
    with np.errstate(invalid="ignore"):
        out[0::2] = soft < np.float32(0.0)
        out[1::2] = np.abs(soft) > np.float32(high_cut)
    return out


class Demux:
    """M17FrameDemux::run, a call per `run(bits)` -> the frames that left in that call as (type, uint8 [frame_bits] in de-interleaved order)"""

    def __init__(self, sync=SYNC, scramble=SCRAMBLE, interleave=INTERLEAVE):
        self.sync = [np.array([(w >> (15 - b)) & 1 for b in range(16)], np.uint8) for w in sync]
        self.scramble, self.interleave, self.nbits = np.asarray(scramble, np.uint8), np.asarray(interleave, np.int64), len(scramble)
        self.delay, self.detect, self.type, self.out_count, self.frame = np.zeros(16, np.uint8), False, 0, 0, np.zeros(len(scramble), np.uint8)

    def run(self, bits):
        bits = np.asarray(bits, np.uint8)
        count, d, frames, i = len(bits), np.concatenate([self.delay, np.asarray(bits, np.uint8)]), [], 0
        while i < count:
            if self.detect:
                if self.out_count >= 16:
                    k = self.out_count - 16
                    self.frame[self.interleave[k]] = d[i] ^ self.scramble[k]
                i += 1
                self.out_count += 1
                if self.out_count >= 16 + self.nbits:
                    self.detect = False
                    frames.append((self.type, self.frame.copy()))
                continue
            hit = [t for t, w in enumerate(self.sync) if np.array_equal(d[i:i + 16], w)]
            if hit:
                self.detect, self.type, self.out_count = True, hit[0], 0
                continue
            i += 1
        self.delay = d[count:count + 16].copy()
        return frames


def records(frames, nbits=368):
    """frames -> the device's records uint8 [n, stride]: [type][0][nbits / 8 bytes, position 0 in the MSB of the first][zero padding to a multiple of 4]"""
    stride = (2 + nbits // 8 + 3) & ~3
    out = np.zeros((len(frames), stride), np.uint8)
    for r, (t, f) in enumerate(frames):
        out[r, 0] = t
        out[r, 2:2 + nbits // 8] = np.packbits(f)
    return out
