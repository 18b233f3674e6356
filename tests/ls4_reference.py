"""numpy restatement of the LabSat 4 families of gsh_packed_format (include/gnss_sdr_hip.h), written from the layout the header states (reference:
gnuradio_blocks/labsat23_source.cc, write_samples_ls4 / read_ls4_data / parse_ls4_data), not from the library's decoder.
A layout is (QUA, regs): regs[s] 64-bit little-endian registers of channel slot s (A, B, C) per round, 0 for a slot that is not recorded.  The DECODER
turns every buffer of a slot into its bit stream (np.unpackbits of the registers, register 0 first, most significant bit first) and cuts that into
fields of 2 QUA bits.  The PACKER goes the other way, from sample codes to the bytes of the file, by laying code bits into a bit array and packing it
into registers: it shares no line with the decoder.  Both follow the stated deviation (bit i of a field at offset `start` is bit 63 - start - i)."""
import numpy as np

LS4_1BIT, LS4_2BIT, LS4_4BIT, LS4_8BIT, LS4_12BIT = 14, 15, 16, 17, 18
FAMILY = {1: LS4_1BIT, 2: LS4_2BIT, 4: LS4_4BIT, 8: LS4_8BIT, 12: LS4_12BIT}
QUAS = (1, 2, 4, 8, 12)
# one slot; three equal slots; slot B alone; BW_DIV 1 / 2 / 4: a 168-byte round.  Every count is a multiple of 3 (QUA 12 takes whole triples)
LAYOUTS = ((6, 0, 0), (6, 6, 6), (0, 6, 0), (12, 6, 3))
ROUNDS = 5


def samples_per_register(qua: int) -> int:
    """whole samples per register; at QUA 12 per triple of registers"""
    return 8 if qua == 12 else 32 // qua


def samples_per_round(qua: int, regs, slot: int) -> int:
    return regs[slot] * 32 // qua


def round_bytes(regs) -> int:
    return 8 * sum(regs)


def value(code: np.ndarray, qua: int) -> np.ndarray:
    """generate_mapping: code < half -> (code + 1) / half, else (code - 2^QUA) / half"""
    half = 1 << (qua - 1)
    code = np.asarray(code, np.int64)
    return np.where(code < half, (code + 1) / half, (code - (1 << qua)) / half)


def decode(data: np.ndarray, qua: int, regs, slot: int) -> np.ndarray:
    """every sample of channel slot `slot` in the bytes `data` (whole rounds) -> complex64 [rounds S]"""
    rb = round_bytes(regs)
    a = np.ascontiguousarray(data).view(np.uint8).reshape(-1, rb)
    lo = 8 * sum(regs[:slot])
    buf = a[:, lo:lo + 8 * regs[slot]].reshape(a.shape[0], regs[slot], 8)
    stream = np.unpackbits(buf[:, :, ::-1], axis=2).reshape(a.shape[0], -1)     # per round: register 0 first, each from bit 63 down
    fields = stream.reshape(a.shape[0], -1, 2, qua).astype(np.int64)             # [round, sample, (I, Q), bit]
    weights = 1 << np.arange(qua - 1, -1, -1)                                    # most significant bit first
    codes = fields @ weights
    return (value(codes[:, :, 0], qua) + 1j * value(codes[:, :, 1], qua)).astype(np.complex64).reshape(-1)


def pack(codes_i, codes_q, qua: int, regs) -> np.ndarray:
    """The packer: codes_i[s], codes_q[s] = the sample codes (0 .. 2^QUA - 1) of slot s, [rounds * S_s] each (ignored for a slot with regs 0) -> the
    bytes of the file.  Round after round, slot after slot, the codes of the round are written I then Q, most significant bit first, into a row of bit
    cells; every 64 cells become one register, the first cell its bit 63, stored little-endian."""
    rounds = None
    for s in range(3):
        if regs[s]:
            r = len(codes_i[s]) // samples_per_round(qua, regs, s)
            assert rounds in (None, r) and len(codes_i[s]) == len(codes_q[s]) == r * samples_per_round(qua, regs, s)
            rounds = r
    out = []
    for rnd in range(rounds):
        for s in range(3):
            if not regs[s]:
                continue
            S = samples_per_round(qua, regs, s)
            cells = np.zeros(64 * regs[s], np.uint64)
            at = 0
            for k in range(rnd * S, (rnd + 1) * S):
                for code in (int(codes_i[s][k]), int(codes_q[s][k])):
                    for bit in range(qua - 1, -1, -1):
                        cells[at] = (code >> bit) & 1
                        at += 1
            assert at == cells.size
            reg = np.zeros(regs[s], np.uint64)
            for cell in cells.reshape(regs[s], 64).T:            # shift the row in from the right: the first cell ends at bit 63
                reg = (reg << np.uint64(1)) | cell
            out.append(reg.astype("<u8").view(np.uint8))
    return np.concatenate(out)
