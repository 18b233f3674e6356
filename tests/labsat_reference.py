"""numpy restatement of the register families of gsh_packed_format (include/gnss_sdr_hip.h): LabSat 2 / 3, LabSat 3 Wideband and SPIR 1-bit, written
from the layout the header states (reference: gnuradio_blocks/labsat23_source.cc, unpack_intspir_1bit_samples.cc), not from the library's decoder.
The decoders work on bit arrays (np.unpackbits of the register, most significant bit first); the LabSat 3 Wideband PACKER below goes the other way,
from sample codes to registers, by placing every code bit at its position in a bit matrix: it shares no line with the decoders.
LabSat 3 Wideband follows the stated deviation from the reference as compiled (bit i of a field at offset `start` is bit 63 - start - i)."""
import numpy as np

LABSAT_2BIT, LABSAT_4BIT, LS3W_1BIT, LS3W_2BIT, LS3W_3BIT, SPIR_1BIT = 8, 9, 10, 11, 12, 13

# samples per 64-bit register by (QUA, CHN): (without, with) digital I/O
LS3W_SPR = {(1, 1): (32, 30), (1, 2): (16, 15), (1, 3): (10, 10),
            (2, 1): (16, 15), (2, 2): (8, 7), (2, 3): (5, 5),
            (3, 1): (10, 10), (3, 2): (5, 5), (3, 3): (3, 3)}
LS3W_LAYOUTS = [(q, c, d) for q in (1, 2, 3) for c in (1, 2, 3) for d in (False, True)]   # the 18 combinations


def ls3w_spr(qua: int, chn: int, dio: bool) -> int:
    return LS3W_SPR[(qua, chn)][1 if dio else 0]


def ls3w_spare(qua: int, chn: int, dio: bool) -> int:
    return 64 - ls3w_spr(qua, chn, dio) * 2 * qua * chn


def _bits_msb_first(values: np.ndarray, width: int) -> np.ndarray:
    """[n] unsigned integers -> [n, width] bits, column 0 = bit width - 1"""
    v = np.asarray(values, np.uint64).reshape(-1, 1)
    shifts = np.arange(width - 1, -1, -1, dtype=np.uint64).reshape(1, -1)
    return ((v >> shifts) & np.uint64(1)).astype(np.int64)


def decode_labsat_2bit(items: np.ndarray) -> np.ndarray:
    """[n] 16-bit items -> complex64 [8 n]: sample i has I = bit 15 - 2i, Q = bit 14 - 2i, value 2 b - 1"""
    b = _bits_msb_first(items, 16)                     # column k = bit 15 - k
    i, q = 2 * b[:, 0::2] - 1, 2 * b[:, 1::2] - 1
    return (i + 1j * q).astype(np.complex64).reshape(-1)


def decode_labsat_4bit(items: np.ndarray) -> np.ndarray:
    """[n] 16-bit items -> complex64 [4 n]: per nibble (from the top) I sign, Q sign, I magnitude, Q magnitude"""
    b = _bits_msb_first(items, 16).reshape(-1, 4, 4)   # [item, sample, (Isign, Qsign, Imag, Qmag)]
    table = np.array([[1, 2], [-2, -1]])                # [sign][magnitude]
    i, q = table[b[:, :, 0], b[:, :, 2]], table[b[:, :, 1], b[:, :, 3]]
    return (i + 1j * q).astype(np.complex64).reshape(-1)


def decode_spir_1bit(words: np.ndarray) -> np.ndarray:
    """[n] 32-bit items -> complex64 [n]: I = bit 0, Q = bit 1, +-32767"""
    w = np.asarray(words, np.uint32)
    i = np.where(w & np.uint32(1), 32767.0, -32767.0)
    q = np.where(w & np.uint32(2), 32767.0, -32767.0)
    return (i + 1j * q).astype(np.complex64)


def ls3w_value(code: np.ndarray, qua: int) -> np.ndarray:
    """generate_mapping: code < half -> (code + 1) / half, else (code - 2^QUA) / half"""
    half = 1 << (qua - 1)
    code = np.asarray(code, np.int64)
    return np.where(code < half, (code + 1) / half, (code - (1 << qua)) / half)


def decode_ls3w(registers: np.ndarray, qua: int, chn: int, dio: bool, channel: int) -> np.ndarray:
    """[n] 64-bit registers -> complex64 [spr n] of RF channel `channel` (0-based)"""
    spr, spare, sft = ls3w_spr(qua, chn, dio), ls3w_spare(qua, chn, dio), 2 * qua * chn
    b = _bits_msb_first(registers, 64)                 # column o = the bit o places below the top
    weights = 1 << np.arange(qua - 1, -1, -1)          # most significant bit first
    out = np.empty((b.shape[0], spr), np.complex64)
    for i in range(spr):
        o = spare + i * sft + 2 * qua * channel
        ci = b[:, o:o + qua] @ weights
        cq = b[:, o + qua:o + 2 * qua] @ weights
        out[:, i] = ls3w_value(ci, qua) + 1j * ls3w_value(cq, qua)
    return out.reshape(-1)


def pack_ls3w(codes_i: np.ndarray, codes_q: np.ndarray, qua: int, chn: int, dio: bool, spare_bits: np.ndarray | None = None) -> np.ndarray:
    """The packer: codes_i, codes_q [chn, n_registers * spr] sample codes (0 .. 2^QUA - 1) -> [n_registers] uint64.  Every register is built as a row
    of 64 bit cells, cell 0 the most significant: the spare cells first (spare_bits [n_registers, spare], zeros when None), then sample after sample,
    within a sample channel after channel, within a channel the I code then the Q code, each code most significant bit first."""
    spr, spare = ls3w_spr(qua, chn, dio), ls3w_spare(qua, chn, dio)
    codes_i = np.asarray(codes_i, np.uint64).reshape(chn, -1, spr)
    codes_q = np.asarray(codes_q, np.uint64).reshape(chn, -1, spr)
    n_reg = codes_i.shape[1]
    cells = []                                          # list of [n_reg] bit columns, in register order
    for k in range(spare):
        cells.append(np.zeros(n_reg, np.uint64) if spare_bits is None else np.asarray(spare_bits, np.uint64)[:, k])
    for s in range(spr):
        for c in range(chn):
            for code in (codes_i[c, :, s], codes_q[c, :, s]):
                for bit in range(qua - 1, -1, -1):
                    cells.append((code >> np.uint64(bit)) & np.uint64(1))
    assert len(cells) == 64
    reg = np.zeros(n_reg, np.uint64)
    for cell in cells:                                  # shift the row in from the right: the first cell ends at bit 63
        reg = (reg << np.uint64(1)) | cell
    return reg


def decode(family: int, data: np.ndarray, rf_channels: int = 1, channel: int = 0, dio: bool = False) -> np.ndarray:
    """every sample of `channel` in the packed bytes `data` (uint8, whole items)"""
    a = np.ascontiguousarray(data).view(np.uint8).reshape(-1)
    if family == LABSAT_2BIT:
        return decode_labsat_2bit(a.view("<u2"))
    if family == LABSAT_4BIT:
        return decode_labsat_4bit(a.view("<u2"))
    if family == SPIR_1BIT:
        return decode_spir_1bit(a.view("<u4"))
    return decode_ls3w(a.view("<u8"), family - LS3W_1BIT + 1, rf_channels, dio, channel)


def samples_per_item(family: int, rf_channels: int = 1, dio: bool = False) -> int:
    if family in (LABSAT_2BIT, LABSAT_4BIT, SPIR_1BIT):
        return {LABSAT_2BIT: 8, LABSAT_4BIT: 4, SPIR_1BIT: 1}[family]
    return ls3w_spr(family - LS3W_1BIT + 1, rf_channels, dio)


def item_bytes(family: int) -> int:
    return 2 if family in (LABSAT_2BIT, LABSAT_4BIT) else 4 if family == SPIR_1BIT else 8
