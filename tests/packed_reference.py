"""Independent numpy restatement of the reference's packed-sample signal sources: each unpack block of
src/algorithms/signal_source/gnuradio_blocks/ ("blocks/" below) and the GNU Radio conversion the adapter puts behind it
(src/algorithms/signal_source/adapters/, "adapters/" below).  GNU Radio is not vendored in the reference, so char_to_float,
interleaved_char_to_complex and interleaved_short_to_complex(vector_input, swap) are restated from their documentation, scale 1: a
plain integer -> float cast, (I, Q) = (x[2k], x[2k+1]), swapped when `swap`.  The block restatements are pinned to the reference's
own compiled blocks by tests/golden/packed_formats.npz (minted by tests/golden/make_golden_packed.py)."""
import numpy as np


def _s2(v):
    """a `signed x : 2` bit-field assigned (c >> k) & 3: two's complement, 0 1 -2 -1 (blocks/unpack_2bit_samples.cc:22-28)"""
    v = np.asarray(v).astype(np.int16) & 3
    return np.where(v >= 2, v - 4, v)


# ---- the unpack blocks (their raw outputs) -------------------------------------------------------------------------------------------


def unpack_2bit_samples(data, big_endian_bytes, item_size, big_endian_items, reverse_interleaving):
    """blocks/unpack_2bit_samples.cc:103-206 on a little-endian host -> int8, 4 per byte"""
    b = np.asarray(data, np.uint8).reshape(-1)
    if item_size > 1 and big_endian_items:            # swap_endian_items_ (:114-115), swapEndianness (:63-80)
        b = b.reshape(-1, item_size)[:, ::-1].reshape(-1)
    fields = np.stack([_s2(b >> (2 * k)) for k in range(4)], axis=1)   # sample_0 .. sample_3 (bits 1:0 .. 7:6)
    if not reverse_interleaving:
        order = [3, 2, 1, 0] if big_endian_bytes else [0, 1, 2, 3]     # :152-177 (swap_endian_bytes_ = big_endian_bytes, :118-120)
    else:
        order = [2, 3, 0, 1] if big_endian_bytes else [1, 0, 3, 2]     # :181-205
    return (2 * fields[:, order] + 1).astype(np.int8).reshape(-1)


def unpack_byte_2bit_cpx_samples(data):
    """blocks/unpack_byte_2bit_cpx_samples.cc:77-89 -> int16, 4 per byte: bits 5:4, 7:6, 1:0, 3:2 (its own I/Q swap)"""
    c = np.asarray(data, np.uint8).reshape(-1)
    return np.stack([2 * _s2(c >> 4) + 1, 2 * _s2(c >> 6) + 1, 2 * _s2(c) + 1, 2 * _s2(c >> 2) + 1], axis=1).astype(np.int16).reshape(-1)


def unpack_byte_4bit_samples(data):
    """blocks/unpack_byte_4bit_samples.cc:44-64 -> int16, low nibble then high nibble, n >= 8 -> 2 (n - 16) + 1, else 2 n + 1"""
    c = np.asarray(data, np.uint8).reshape(-1).astype(np.int16)
    nib = np.stack([c & 15, (c >> 4) & 15], axis=1)
    return np.where(nib >= 8, 2 * (nib - 16) + 1, 2 * nib + 1).astype(np.int16).reshape(-1)


def unpack_byte_2bit_samples(data):
    """blocks/unpack_byte_2bit_samples.cc:50-64 (Nsr) -> float32, 4 per byte: bits 1:0, 3:2, 5:4, 7:6 as signed fields, -2 .. 1"""
    c = np.asarray(data, np.uint8).reshape(-1)
    return np.stack([_s2(c >> (2 * k)) for k in range(4)], axis=1).astype(np.float32).reshape(-1)


def unpack_ntlab_2bit_samples(data, nchannels=4):
    """blocks/unpack_ntlab_2bit_samples.cc:57-77 with 4 channels -> float32 [4, n]: channel n reads bits 7-2n (magnitude), 6-2n (sign)"""
    assert nchannels == 4, "1 and 2 channels read past the block's input (unpack_ntlab_2bit_samples.cc:38,57-77)"
    b = np.asarray(data, np.uint8).reshape(-1).astype(np.int16)
    out = []
    for n in range(4):
        shift = 2 * (3 - n)
        mag = np.where((b >> (shift + 1)) & 1, 3, 1)
        out.append(np.where((b >> shift) & 1, mag, -mag).astype(np.float32))
    return np.stack(out)


# ---- GNU Radio's conversions (documentation, scale 1) ----------------------------------------------------------------------------------


def char_to_float(x):
    return np.asarray(x).astype(np.float32)


def interleaved_to_complex(x, swap=False):
    """interleaved_char_to_complex(false) / interleaved_short_to_complex(false, swap): (x[2k], x[2k+1]) -> I + jQ, swapped when `swap`"""
    x = np.asarray(x).astype(np.float32)
    i, q = (x[1::2], x[0::2]) if swap else (x[0::2], x[1::2])
    out = np.empty(i.size, np.complex64)
    out.real, out.imag = i, q
    return out


# ---- the signal sources: packed bytes -> what the source hands the flowgraph ---------------------------------------------------------


def source_output(implementation, data, **properties):
    """complex64 [n] for the complex sources, float32 [n] for Two_Bit_Packed real / Nsr, float32 [4, n] for NTLab.  Property names and
    defaults of the reference adapters."""
    d = np.asarray(data, np.uint8).reshape(-1)
    flag = lambda v: (v.strip().lower() in ("true", "1")) if isinstance(v, str) else bool(v)
    if implementation == "Two_Bit_Packed_File_Signal_Source":
        # adapters/two_bit_packed_file_signal_source.cc:38-41 (defaults), :54-101 (item size, complexity), :118-136 (blocks)
        item_type = properties.get("item_type", "byte")
        sample_type = properties.get("sample_type", "real")
        bei, beb = flag(properties.get("big_endian_items", True)), flag(properties.get("big_endian_bytes", False))
        item_size = 2 if (item_type == "short" and bei) else 1        # little-endian shorts are read as bytes (:63-77)
        u = unpack_2bit_samples(d, beb, item_size, bei, sample_type == "qi")
        return char_to_float(u) if sample_type == "real" else interleaved_to_complex(u)
    if implementation == "Two_Bit_Cpx_File_Signal_Source":
        return interleaved_to_complex(unpack_byte_2bit_cpx_samples(d), swap=True)   # adapters/two_bit_cpx_file_signal_source.cc:72-81
    if implementation == "Four_Bit_Cpx_File_Signal_Source":
        qi = properties.get("sample_type", "iq") == "qi"                             # adapters/four_bit_cpx_file_signal_source.cc:38-55,118-121
        return interleaved_to_complex(unpack_byte_4bit_samples(d), swap=qi)
    if implementation == "Nsr_File_Signal_Source":
        return unpack_byte_2bit_samples(d)                                            # adapters/nsr_file_signal_source.cc:69-76
    if implementation == "NTLab_File_Signal_Source":
        return unpack_ntlab_2bit_samples(d, int(properties.get("RF_channels", 4)))    # adapters/ntlab_file_signal_source.cc:41-45,100-127
    raise ValueError(implementation)


# every family x option the device path supports: (implementation, properties)
COMPLEX_SOURCES = [("Two_Bit_Packed_File_Signal_Source", dict(item_type=it, sample_type=st, big_endian_bytes=beb, big_endian_items=bei))
                   for it in ("byte", "short") for st in ("iq", "qi") for beb in (False, True) for bei in ((False, True) if it == "short" else (True,))] + [
                  ("Two_Bit_Cpx_File_Signal_Source", {}),
                  ("Four_Bit_Cpx_File_Signal_Source", dict(sample_type="iq")),
                  ("Four_Bit_Cpx_File_Signal_Source", dict(sample_type="qi"))]
REAL_SOURCES = [("Two_Bit_Packed_File_Signal_Source", dict(item_type=it, sample_type="real", big_endian_bytes=beb, big_endian_items=bei))
                for it in ("byte", "short") for beb in (False, True) for bei in ((False, True) if it == "short" else (True,))] + [
               ("Nsr_File_Signal_Source", {}),
               ("NTLab_File_Signal_Source", dict(RF_channels=4))]


def source_id(src):
    impl, props = src
    return impl.split("_File_")[0] + "".join(f"-{k}={v}" for k, v in sorted(props.items()))
