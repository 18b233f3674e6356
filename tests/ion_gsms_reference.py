"""Numpy restatement of the ION_GSMS layout (include/gnss_sdr_hip.h, "ION GNSS SDR metadata standard") and an independent packer: the checker of
gsh_ion_decode_host and, through it, of the device unpack.  The restatement works on the bits that np.unpackbits returns and forms every value from
bit weights; the packer builds a chunk as one Python integer.  Neither shares arithmetic with csrc/ion_gsms.h."""
from __future__ import annotations

import numpy as np

SIGN, OB, SM, MS, TC, OG, OBA, SMA, MSA, TCA, OGA, FP = range(12)
ENCODING_NAMES = ["SIGN", "OB", "SM", "MS", "TC", "OG", "OBA", "SMA", "MSA", "TCA", "OGA"]
REAL, IQ, QI = 0, 1, 2


def chunk(size_word, count_words, streams, big_endian=0, padding=0, shift=0):
    return {"size_word": size_word, "count_words": count_words, "big_endian": big_endian, "shift": shift, "padding": padding,
            "n_streams": len(streams), "streams": list(streams)}


def stream(packed_bits, rate_factor, quantization, encoding, format=REAL, alignment=0, lump_shift=0, negate=0, name=None):
    return {"packed_bits": packed_bits, "rate_factor": rate_factor, "quantization": quantization, "encoding": encoding, "format": format,
            "alignment": alignment, "lump_shift": lump_shift, "negate": negate, "name": name}


def flat(chunks):
    return [s for c in chunks for s in c["streams"]]


def cycle_bytes(chunks):
    return sum(c["size_word"] * c["count_words"] for c in chunks)


def field_bits(s):
    return s["packed_bits"] // (s["rate_factor"] * (1 if s["format"] == REAL else 2))


def fields_per_cycle(s):
    return s["rate_factor"] * (1 if s["format"] == REAL else 2)


def code_bits(s):
    return field_bits(s) if s["alignment"] == 0 else s["quantization"]


def _weights(n):
    return (1 << np.arange(n - 1, -1, -1)).astype(np.int64)


def values(bits: np.ndarray, encoding: int) -> np.ndarray:
    """bits[..., q] of 0 / 1, most significant first -> the value of each code, from bit weights"""
    b = bits.astype(np.int64)
    q = b.shape[-1]
    if encoding in (OG, OGA):
        b = np.bitwise_xor.accumulate(b, axis=-1)      # Gray -> binary: every bit is the parity of the Gray bits at and above it
    if encoding == SIGN:
        assert q == 1
        return 1 - 2 * b[..., 0]
    if encoding in (OB, OG):
        return b @ _weights(q) - (1 << (q - 1))
    if encoding in (OBA, OGA):
        return 2 * (b @ _weights(q)) - ((1 << q) - 1)
    if encoding in (TC, TCA):
        w = _weights(q)
        w[0] = -w[0]                                    # two's complement: the leading bit weighs -2^(q-1)
        v = b @ w
        return v if encoding == TC else 2 * v + 1
    if encoding in (SM, SMA):
        m = b[..., 1:] @ _weights(q - 1) if q > 1 else np.zeros(b.shape[:-1], np.int64)
        sign = b[..., 0]
    else:
        assert encoding in (MS, MSA)
        m = b[..., :-1] @ _weights(q - 1) if q > 1 else np.zeros(b.shape[:-1], np.int64)
        sign = b[..., -1]
    if encoding in (SMA, MSA):
        m = 2 * m + 1
    return np.where(sign == 1, -m, m)


def chunk_bits(chunks, data: np.ndarray):
    """per chunk: the bit stream of every cycle, bits[cycle, bit], words in ascending order and each from its most significant bit down"""
    cb = cycle_bytes(chunks)
    d = np.asarray(data, np.uint8).reshape(-1, cb)
    out, off = [], 0
    for c in chunks:
        w, n = c["size_word"], c["count_words"]
        words = d[:, off:off + w * n].reshape(-1, n, w)
        if not c["big_endian"]:
            words = words[:, :, ::-1]
        out.append(np.unpackbits(np.ascontiguousarray(words).reshape(d.shape[0], w * n), axis=1))
        off += w * n
    return out


def decode(chunks, data: np.ndarray, index: int) -> np.ndarray:
    """every sample of stream `index` (counted over the flattened streams) in the whole cycles of `data`: float32 (real) or complex64"""
    bits = chunk_bits(chunks, data)
    at = 0
    for c, cbits in zip(chunks, bits):
        pad = cbits.shape[1] - sum(s["packed_bits"] for s in c["streams"])
        assert pad >= 0
        pos = pad if c["padding"] == 1 else 0
        for s in c["streams"]:
            if at == index:
                w, q = field_bits(s), code_bits(s)
                f = cbits[:, pos:pos + s["packed_bits"]].reshape(cbits.shape[0], fields_per_cycle(s), w)
                code = f[:, :, :q] if s["alignment"] in (0, 1) else f[:, :, w - q:]
                v = values(code, s["encoding"])
                if s["format"] == REAL:
                    return (-v if s["negate"] & 1 else v).reshape(-1).astype(np.float32)
                v = v.reshape(v.shape[0], -1, 2)
                i, q_ = (v[..., 0], v[..., 1]) if s["format"] == IQ else (v[..., 1], v[..., 0])
                i = -i if s["negate"] & 1 else i
                q_ = -q_ if s["negate"] & 2 else q_
                return (i.reshape(-1).astype(np.float32) + 1j * q_.reshape(-1).astype(np.float32)).astype(np.complex64)
            pos += s["packed_bits"]
            at += 1
    raise IndexError(index)


def pack(chunks, n_cycles: int, fields: dict, rng) -> np.ndarray:
    """bytes of n_cycles cycles in which stream i holds the fields fields[i][cycle][j] (whole fields of w bits, as Python ints); every other stream and
    every padding bit is random.  A chunk is assembled as one integer, most significant bit first, and cut into words."""
    out = bytearray()
    for cyc in range(n_cycles):
        at = 0
        for c in chunks:
            total = 8 * c["size_word"] * c["count_words"]
            used = sum(s["packed_bits"] for s in c["streams"])
            pad = total - used
            acc, nbits = 0, 0
            if c["padding"] == 1 and pad:
                acc, nbits = int.from_bytes(rng.bytes((pad + 7) // 8), "big") >> (-pad % 8), pad
            for s in c["streams"]:
                w = field_bits(s)
                for j in range(fields_per_cycle(s)):
                    v = int(fields[at][cyc][j]) if at in fields else int(rng.integers(0, 1 << w))
                    assert 0 <= v < (1 << w)
                    acc, nbits = (acc << w) | v, nbits + w
                at += 1
            if nbits < total:                           # tail padding (or all of it where the chunk has no head padding)
                rest = total - nbits
                acc = (acc << rest) | (int.from_bytes(rng.bytes((rest + 7) // 8), "big") >> (-rest % 8))
            raw = acc.to_bytes(total // 8, "big")
            w = c["size_word"]
            for k in range(0, len(raw), w):
                out += raw[k:k + w] if c["big_endian"] else raw[k:k + w][::-1]
    return np.frombuffer(bytes(out), np.uint8).copy()


def field_to_code(s, field: int) -> int:
    w, q = field_bits(s), code_bits(s)
    return field >> (w - q) if s["alignment"] in (0, 1) else field & ((1 << q) - 1)


def value_of(encoding: int, q: int, code: int) -> int:
    """one code -> its value, through values()"""
    bits = np.array([(code >> (q - 1 - i)) & 1 for i in range(q)], np.uint8)
    return int(values(bits, encoding))


def encoding_row(encoding: int, q: int) -> list:
    return [value_of(encoding, q, c) for c in range(1 << q)]


# ---------------------------------------------------------------------------------------------------------------- the grid of layouts
def _quantization(enc, w, alignment):
    if enc == SIGN:
        return 1
    return w if alignment == 0 else max(1, w - enc % 3)


def grid_chunk(size_word, big_endian, head, w, kind, salt=0, encodings=range(11)):
    """one chunk that holds a stream of every encoding (of `encodings`) at field width w and of kind `kind`, alignments cycling with (encoding + w + salt), an unselected
    stream of 5 bits between each two of them (so that fields start at every bit position and straddle words), with head padding or without"""
    streams = []
    per = 1 if kind == REAL else 2
    for enc in encodings:
        alignment = (enc + w + salt) % 3
        if enc == SIGN and w > 1 and alignment == 0:
            alignment = 1 + (w + salt) % 2
        rate = 3 if enc % 2 else 2
        negate = (enc + w) % (4 if per == 2 else 2)
        streams.append(stream(w * per * rate, rate, _quantization(enc, w, alignment), enc, kind, alignment, 0, negate, name=f"{ENCODING_NAMES[enc]}{w}"))
        streams.append(stream(5, 1, 3, OB, REAL, 2, name=f"skip{enc}"))
    used = sum(s["packed_bits"] for s in streams)
    word = 8 * size_word
    count = (used + (3 if head else 0) + word - 1) // word
    if head and count * word == used:
        count += 1
    return chunk(size_word, count, streams, big_endian, 1 if head else 0)


def random_fields(chunks, n_cycles, rng):
    """fields for every stream, chosen so that the extreme codes occur: all zeros, all ones, then random"""
    out = {}
    for i, s in enumerate(flat(chunks)):
        w, n = field_bits(s), fields_per_cycle(s)
        f = rng.integers(0, 1 << w, (n_cycles, n), dtype=np.int64)
        f[0, 0] = 0
        f[-1, -1] = (1 << w) - 1
        if n_cycles > 1:
            f[1, 0] = 1 << (w - 1)
        out[i] = f
    return out


def windows(rate, total):
    """(first, n): the whole block, and windows that start and end inside a cycle"""
    out = [(0, total)]
    for first, n in ((1, total - 2), (rate + 1, 2 * rate - 1), (rate - 1, 1), (total - 1, 1), (2 * rate - 1, rate + 2)):
        if n > 0 and first >= 0 and first + n <= total:
            out.append((first, n))
    return out
