"""numpy float32 restatement of the Galileo telemetry page decoder (gnss-sdr_amd/csrc/viterbi_acs.h says the same in C++): deinterleaver, signs, the K = 7
rate 1/2 add-compare-select step operation for operation as viterbi_decoder.cc:59-104, trace-back, bit-serial CRC-24Q, the clipped preamble correlation,
and a job-table engine with the interface of gnss_sdr_amd.telemetry.TelemetryDecoder (so GalileoFrameSync runs on it without a device).  Also the ICD
encoder the tests build their pages with (convolutional code with G2 inverted, tail of 6 zeros, 8-row block interleaver, CRC-24Q).

Two metric modes, as the library: "full" (both symbols of a pair, every page from state 0 alone) and "reference" (rec[1] = 0 and the metrics carried from
page to page, the reference as it runs)."""
import functools
import os

import numpy as np

F32 = np.float32
FIXTURE_FRAMES = (("inav", 1), ("fnav", 2), ("cnav", 3))  # names in tests/golden/viterbi.npz (make_golden_viterbi.py), frame types


@functools.lru_cache(maxsize=1)
def fixture():
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "viterbi.npz"))
    return {k: z[k] for k in z.files}


@functools.lru_cache(maxsize=None)
def fixture_decoded(metric, reused):
    """the restatement over every fixture page, computed once: {name: uint8 [n, bits]}; reused: one decoder over a length's pages in sequence"""
    out = {}
    for name, ft in FIXTURE_FRAMES:
        sym = fixture()[name + "__sym"]
        carry, rows = None, []
        for page in sym:
            bits, end = viterbi(soft_values(page, ft), GEOMETRY[ft]["info_bits"], metric, carry if (reused and metric == "reference") else None)
            carry = end
            rows.append(bits)
        out[name] = np.array(rows)
    return out


MAXLOG = F32(1e7)
GEOMETRY = {
    1: dict(symbols=240, steps=120, info_bits=114, rows=8, cols=30, preamble="0101100000", period=250, required=510),
    2: dict(symbols=488, steps=244, info_bits=238, rows=8, cols=61, preamble="101101110000", period=500, required=512),
    3: dict(symbols=984, steps=492, info_bits=486, rows=8, cols=123, preamble="1011011101110000", period=1000, required=1016),
}
JOB_INVERT, JOB_CRC_CONTINUE, JOB_INAV_AUTO = 1, 2, 4
CRC_POLY = 0x864CFB


def _parity(w):
    return bin(w).count("1") & 1


def out_symbol(inp, state):
    word = (inp << 6) ^ state
    return (_parity(word & 121) << 1) + _parity(word & 91)


_S = np.arange(64)
_PRED = 2 * (_S & 31)
_SYM_LO = np.array([out_symbol(s >> 5, 2 * (s & 31)) for s in range(64)])
_SYM_HI = np.array([out_symbol(s >> 5, 2 * (s & 31) + 1) for s in range(64)])


def soft_values(page, frame_type, invert=False):
    """the decoder's input: galileo_telemetry_decoder_gs.cc:1033-1046 (180 deg), :352-361 (deinterleaver), :371-377 (NOT gate of G2)"""
    g = GEOMETRY[frame_type]
    x = np.asarray(page, F32)
    assert x.shape == (g["symbols"],)
    if invert:
        x = -x
    soft = x.reshape(g["rows"], g["cols"]).T.reshape(-1).copy()
    soft[1::2] = -soft[1::2]
    return soft


def _gamma(sym, rec0, rec1):
    rm = np.zeros(64, F32)
    rm = np.where(sym & 1, rm + rec1, rm).astype(F32)
    rm = np.where(sym & 2, rm + rec0, rm).astype(F32)
    return rm


def viterbi(soft, info_bits, metric, prev=None):
    """-> (bits uint8[info_bits], the normalised metrics after the last step).  prev: the 64 metrics to start from (element 0 is set to 0), None: -1e7"""
    steps = len(soft) // 2
    prev = np.full(64, -MAXLOG, F32) if prev is None else np.array(prev, F32)
    prev[0] = F32(0)
    dec = np.zeros((steps, 64), np.uint8)
    for t in range(steps):
        rec0 = F32(soft[2 * t])
        rec1 = F32(0) if metric == "reference" else F32(soft[2 * t + 1])
        m_lo = prev[_PRED] + _gamma(_SYM_LO, rec0, rec1)
        nxt = np.where(m_lo > -MAXLOG, m_lo, -MAXLOG).astype(F32)
        m_hi = prev[_PRED + 1] + _gamma(_SYM_HI, rec0, rec1)
        d = m_hi > nxt
        nxt = np.where(d, m_hi, nxt).astype(F32)
        dec[t] = d
        prev = (nxt - nxt.max()).astype(F32)
    bits = np.zeros(info_bits, np.uint8)
    state = 0
    for t in range(steps - 1, -1, -1):
        if t < info_bits:
            bits[t] = state >> 5
        state = 2 * (state & 31) + int(dec[t, state])
    return bits, prev


def crc24q(bits, reg=0):
    for b in bits:
        top = (reg >> 23) & 1
        reg = (reg << 1) & 0xFFFFFF
        if top ^ int(b):
            reg ^= CRC_POLY
    return reg


def pack_bits(bits):
    """MSB first into 16 uint32 words"""
    padded = np.zeros(512, np.uint8)
    padded[:len(bits)] = bits
    return np.packbits(padded).view(">u4").astype(np.uint32)


def unpack_bits(words, info_bits):
    return np.unpackbits(np.asarray(words, np.uint32).astype(">u4").view(np.uint8))[:info_bits]


def preamble_corr(symbols, frame_type):
    """galileo_telemetry_decoder_gs.cc:962-972 at every position; 0 where the window leaves the block"""
    pre = np.array([1 if c == "1" else -1 for c in GEOMETRY[frame_type]["preamble"]], np.int32)
    x = np.asarray(symbols, F32)
    clipped = np.where(x < 0, -1, 1).astype(np.int32)
    out = np.zeros(len(x), np.int8)
    n = len(x) - len(pre) + 1
    if n > 0:
        win = np.lib.stride_tricks.sliding_window_view(clipped, len(pre))
        out[:n] = (win * pre).sum(axis=1)
    return out


class NumpyTelemetryDecoder:
    """gsh_tlm_* on the host: the interface of gnss_sdr_amd.telemetry.TelemetryDecoder"""

    def __init__(self, n_channels, metric="full"):
        assert metric in ("full", "reference")
        self.n_channels, self.metric = n_channels, metric
        self.metrics = [None] * n_channels
        self.chain = [0] * n_channels

    def channel_reset(self, channel):
        self.metrics[channel] = None
        self.chain[channel] = 0

    def preamble_scan(self, frame_type, symbols):
        return preamble_corr(symbols, frame_type)

    def decode_pages(self, symbols, jobs):
        symbols = np.asarray(symbols, F32)
        out = []
        for job in jobs:
            ch, ft, off = job["channel"], job["frame_type"], job["symbol_offset"]
            flags = job.get("flags", 0)
            g = GEOMETRY[ft]
            assert 0 <= ch < self.n_channels and off + g["symbols"] <= len(symbols)
            soft = soft_values(symbols[off:off + g["symbols"]], ft, bool(flags & JOB_INVERT))
            bits, end = viterbi(soft, g["info_bits"], self.metric, self.metrics[ch] if self.metric == "reference" else None)
            if self.metric == "reference":
                self.metrics[ch] = end
            cont, n_bits, check = bool(flags & JOB_CRC_CONTINUE), job.get("crc_bits", 0), bool(job.get("crc_check", 0))
            if flags & JOB_INAV_AUTO:
                odd = bool(bits[0])
                cont, n_bits, check = odd, (82 if odd else 114), odd
            reg = crc24q(bits[:n_bits], self.chain[ch] if cont else 0)
            self.chain[ch] = reg
            ok = -1
            if check:
                ok = int(int("".join(str(int(b)) for b in bits[n_bits:n_bits + 24]), 2) == reg)
            out.append(dict(bits=bits, words=pack_bits(bits), crc_register=reg, crc_ok=ok))
        return out

    def close(self):
        pass


# ---- the transmitter's side, for the tests' own pages -----------------------------------------------------------------------------------------
def conv_encode(info):
    """info bits + 6 tail zeros through G1 = 171o, G2 = 133o inverted (Galileo OS SIS ICD figure 13); the shift register holds the newest bit in bit 6"""
    out = []
    state = 0
    for b in list(info) + [0] * 6:
        word = (int(b) << 6) ^ state
        out += [_parity(word & 121), _parity(word & 91) ^ 1]
        state = word >> 1
    return np.array(out, np.uint8)


def encode_page(info, frame_type):
    """information bits -> the symbols after the preamble as transmitted (+1 for a 1): coded, then written column by column into the 8-row block and
    read out row by row"""
    g = GEOMETRY[frame_type]
    assert len(info) == g["info_bits"]
    coded = conv_encode(info)
    tx = coded.reshape(g["cols"], g["rows"]).T.reshape(-1)
    return (2.0 * tx - 1.0).astype(F32)


def with_crc(payload):
    """payload bits followed by their CRC-24Q, MSB first"""
    reg = crc24q(payload)
    return np.concatenate([np.asarray(payload, np.uint8), np.array([(reg >> (23 - k)) & 1 for k in range(24)], np.uint8)])


def preamble_symbols(frame_type):
    return np.array([1.0 if c == "1" else -1.0 for c in GEOMETRY[frame_type]["preamble"]], F32)


def inav_word(rng, good=True):
    """-> (even part, odd part), 114 bits each: 196 bits of word (even starts with 0, odd with 1), CRC-24Q, 8 spare bits; good=False: one payload bit
    flipped after the CRC was formed"""
    word = with_crc(np.concatenate([[0], rng.integers(0, 2, 113), [1], rng.integers(0, 2, 81)]).astype(np.uint8))
    if not good:
        word[50] ^= 1
    return word[:114].copy(), np.concatenate([word[114:], np.zeros(8, np.uint8)])


def nav_page(rng, frame_type, good=True):
    """an F/NAV (214 + 24) or C/NAV (462 + 24) page"""
    page = with_crc(rng.integers(0, 2, GEOMETRY[frame_type]["info_bits"] - 24).astype(np.uint8))
    if not good:
        page[5] ^= 1
    return page


def stream(frame_type, pages):
    """preamble + coded page, page after page, as symbols of unit amplitude"""
    return np.concatenate([np.concatenate([preamble_symbols(frame_type), encode_page(p, frame_type)]) for p in pages])
