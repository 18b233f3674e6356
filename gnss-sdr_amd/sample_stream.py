"""Python face of gsh_stream_* (include/gnss_sdr_hip.h): the device-resident IF sample ring, for tests and bench."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import GSH_ITEM_BYTE, GSH_ITEM_GR_COMPLEX, GSH_ITEM_SHORT, check, fptr

ITEM_TYPES = {"gr_complex": GSH_ITEM_GR_COMPLEX, "ishort": GSH_ITEM_SHORT, "cshort": GSH_ITEM_SHORT, "ibyte": GSH_ITEM_BYTE, "cbyte": GSH_ITEM_BYTE}
_NP = {GSH_ITEM_GR_COMPLEX: np.complex64, GSH_ITEM_SHORT: np.int16, GSH_ITEM_BYTE: np.int8}


def _flag(v) -> int:
    """a boolean property as the reference's configuration reads it (true / false, or a Python bool)"""
    if isinstance(v, str):
        if v.strip().lower() not in ("true", "false", "1", "0"):
            raise ValueError(f"not a boolean: {v!r}")
        return int(v.strip().lower() in ("true", "1"))
    return int(bool(v))


class PackedFormat:
    """gsh_packed_format: packed 2-bit / 4-bit front-end samples, unpacked on the device the way the reference's signal source unpacks them
    (include/gnss_sdr_hip.h).  Build it from the source's configuration with from_signal_source()."""
    TWO_BIT, TWO_BIT_CPX, FOUR_BIT_CPX, NSR, NTLAB, GSS6450_2BIT, GSS6450_4BIT = 1, 2, 3, 4, 5, 6, 7
    # the register families: LabSat 2 / 3 (16-bit items), LabSat 3 Wideband (64-bit registers, QUA 1 .. 3) and SPIR (32-bit items).  Their layout is in
    # the recording, not in the configuration: from_labsat_header(), from_ls3w_ini()
    LABSAT_2BIT, LABSAT_4BIT, LS3W_1BIT, LS3W_2BIT, LS3W_3BIT, SPIR_1BIT = 8, 9, 10, 11, 12, 13
    # LabSat 4 (64-bit registers in rounds of one buffer per channel slot, QUA 1 / 2 / 4 / 8 / 12): ls4(), from_ls4_ini()
    LS4_1BIT, LS4_2BIT, LS4_4BIT, LS4_8BIT, LS4_12BIT = 14, 15, 16, 17, 18
    LS4_QUA = {1: LS4_1BIT, 2: LS4_2BIT, 4: LS4_4BIT, 8: LS4_8BIT, 12: LS4_12BIT}
    DIGITAL_IO = 1   # flags bit of the LS3W families: digital I/O was recorded beside the RF channels
    LS3W_SAMPLES_PER_REGISTER = {(1, 1): (32, 30), (1, 2): (16, 15), (1, 3): (10, 10), (2, 1): (16, 15), (2, 2): (8, 7), (2, 3): (5, 5),
                                 (3, 1): (10, 10), (3, 2): (5, 5), (3, 3): (3, 3)}   # (QUA, CHN): (without, with) digital I/O
    REAL, IQ, QI = 0, 1, 2
    IMPLEMENTATIONS = {"Two_Bit_Packed_File_Signal_Source": TWO_BIT, "Two_Bit_Cpx_File_Signal_Source": TWO_BIT_CPX,
                       "Four_Bit_Cpx_File_Signal_Source": FOUR_BIT_CPX, "Nsr_File_Signal_Source": NSR, "NTLab_File_Signal_Source": NTLAB,
                       "Spir_GSS6450_File_Signal_Source": GSS6450_4BIT,   # (adc_bits picks GSS6450_2BIT / GSS6450_4BIT)
                       "Spir_File_Signal_Source": SPIR_1BIT}
    SAMPLE_TYPES = {"real": REAL, "iq": IQ, "qi": QI}

    def __init__(self, family: int, sample_type: int = REAL, item_size: int = 1, big_endian_bytes: bool = False, big_endian_items: bool = False,
                 rf_channels: int = 0, channel: int = 0, flags: int = 0):
        self.family, self.sample_type, self.item_size = int(family), int(sample_type), int(item_size)
        self.big_endian_bytes, self.big_endian_items = int(big_endian_bytes), int(big_endian_items)
        self.rf_channels, self.channel, self.flags = int(rf_channels), int(channel), int(flags)

    @classmethod
    def from_signal_source(cls, implementation: str, **properties) -> "PackedFormat":
        """The format of SignalSource.implementation = `implementation` with the reference's property names and defaults
        (two_bit_packed_file_signal_source.cc:38-41: item_type byte, sample_type real, big_endian_items true, big_endian_bytes false;
        four_bit_cpx_file_signal_source.cc:38: sample_type iq; ntlab_file_signal_source.cc:41-42: RF_channels 4).  `channel` (not a reference
        property) picks the RF channel of an NTLab stream for unpack_device / a packed FirFilter.  Spir_GSS6450_File_Signal_Source
        (spir_gss6450_file_signal_source.cc:46-55): adc_bits 4, total_channels 1, sel_ch 1, endian false; the single-channel calls take band
        sel_ch - 1.  Spir_File_Signal_Source: the 1-bit SPIR family; its item_type falls back to int whatever it says (spir_file_signal_source.cc:50-58).
        Labsat_Signal_Source: the layout is in the recording, so give the file's first 1 024 bytes as header= (LabSat 2 / 3) or the text of the .ini beside
        a .ls3w file as ini= (LabSat 3 Wideband), with the reference's selected_channel and digital_io_enabled; a filename= that ends in .ls4 makes ini=
        the .ini of a LabSat 4 recording (the reference tells the generations apart by the extension, labsat23_source.cc:333-361).  Other properties of
        the source are ignored."""
        if implementation == "Labsat_Signal_Source":
            sel = int(properties.get("selected_channel", 1))
            if properties.get("header") is not None:
                return cls.from_labsat_header(properties["header"], sel)[0]
            if properties.get("ini") is not None and str(properties.get("filename", "")).endswith((".ls4", ".LS4")):   # (generate_filename, :351-354)
                return cls.from_ls4_ini(properties["ini"], sel)
            if properties.get("ini") is not None:
                return cls.from_ls3w_ini(properties["ini"], sel, bool(_flag(properties.get("digital_io_enabled", False))))
            raise ValueError("Labsat_Signal_Source: the layout is in the recording, not in the configuration: pass header= (the file's first 1 024 bytes) or "
                             "ini= (the text of the .ini of a .ls3w file), or call PackedFormat.from_labsat_header() / from_ls3w_ini()")
        if implementation not in cls.IMPLEMENTATIONS:
            raise ValueError(f"{implementation!r} is not a packed signal source ({', '.join(cls.IMPLEMENTATIONS)})")
        fam = cls.IMPLEMENTATIONS[implementation]
        if implementation == "Spir_GSS6450_File_Signal_Source":
            adc_bits = int(properties.get("adc_bits", 4))
            if adc_bits not in (2, 4):
                raise ValueError(f"adc_bits {adc_bits}: the reference unpacks 2 and 4 only (unpack_spir_gss6450_samples.cc:44-104)")
            return cls(cls.GSS6450_2BIT if adc_bits == 2 else cls.GSS6450_4BIT, cls.IQ, 4, False, _flag(properties.get("endian", False)),
                       rf_channels=int(properties.get("total_channels", 1)), channel=int(properties.get("sel_ch", 1)) - 1)
        if fam == cls.SPIR_1BIT:
            return cls(fam, cls.IQ, 4)
        item_type = properties.get("item_type", "byte")
        if item_type not in (("byte", "short") if fam == cls.TWO_BIT else ("byte",)):
            raise ValueError(f"item_type {item_type!r} is not supported by {implementation}")
        if fam == cls.TWO_BIT:
            st = properties.get("sample_type", "real")
            return cls(fam, cls.SAMPLE_TYPES[st], 2 if item_type == "short" else 1, _flag(properties.get("big_endian_bytes", False)),
                       _flag(properties.get("big_endian_items", True)))
        if fam == cls.FOUR_BIT_CPX:
            st = properties.get("sample_type", "iq")
            if st not in ("iq", "qi"):
                raise ValueError(f"sample_type {st!r} is not iq / qi")
            return cls(fam, cls.SAMPLE_TYPES[st])
        if fam == cls.NTLAB:
            return cls(fam, cls.REAL, rf_channels=int(properties.get("RF_channels", 4)), channel=int(properties.get("channel", 0)))
        return cls(fam, cls.IQ if fam == cls.TWO_BIT_CPX else cls.REAL)

    @classmethod
    def from_labsat_header(cls, header: bytes, selected_channel: int = 1) -> "tuple[PackedFormat, int]":
        """(format, data offset) of a LabSat 2 / LabSat 3 file from its header, read the way the reference reads it (parse_header,
        gnuradio_blocks/labsat23_source.cc:363-583): bytes 0-7 zero, 8-10 "LS2" / "LS3", 11 sub-version, 12-15 header length (little-endian: where the
        samples start), 16-17 section id 2, 18-21 section length, 22 reference clock, 23 bits per sample (2 / 4), 24 channel selector (1..4; 0 = A + B is
        refused as the reference refuses it, :496-500), 25-27 informational.  ValueError for anything the reference refuses."""
        h = bytes(header)
        if len(h) < 28:
            raise ValueError(f"a LabSat header of {len(h)} bytes: at least 28 are read")
        if any(h[:8]):
            raise ValueError("no LabSat preamble: bytes 0-7 of the header are not zero")
        if h[8:11] not in (b"LS2", b"LS3"):
            raise ValueError(f"no LabSat version in the header: bytes 8-10 are {h[8:11]!r}, not LS2 / LS3")
        data_offset = int.from_bytes(h[12:16], "little")
        section_id = int.from_bytes(h[16:18], "little")
        if section_id != 2:
            raise ValueError(f"LabSat header: section id {section_id}, section 2 is not available")
        bits, selector = h[23], h[24]
        if bits not in (2, 4):
            raise ValueError(f"LabSat header: unknown bits per sample {bits} (2 or 4)")
        if selector > 4:
            raise ValueError(f"LabSat header: unknown channel selector {selector}")
        if int(selected_channel) == 2 and selector != 0:
            raise ValueError("selected_channel 2, but the file has only one channel")
        if selector == 0:
            raise ValueError("the file holds channels A + B: more than one channel is not supported for LabSat 2 / 3 files")
        if int(selected_channel) != 1:
            raise ValueError(f"selected_channel {selected_channel}: a LabSat 2 / 3 file carries one RF channel")
        return cls(cls.LABSAT_2BIT if bits == 2 else cls.LABSAT_4BIT, cls.IQ, 2), data_offset

    @classmethod
    def from_ls3w_ini(cls, text: str, selected_channel: int = 1, digital_io_enabled: bool = False) -> "PackedFormat":
        """The format of a LabSat 3 Wideband (.ls3w) recording from the text of the .ini file beside it, read the way the reference reads it (read_ls3w_ini,
        gnuradio_blocks/labsat23_source.cc:678-787): [config] QUA (else QUAN_A), CHN and SFT; QUA above 3 or CHN above 3 is refused; an SFT other than
        2 QUA CHN is replaced by it (:780-784).  The single-channel calls take RF channel selected_channel - 1."""
        import configparser
        ini = configparser.ConfigParser(strict=False, interpolation=None)
        ini.optionxform = str
        ini.read_string(text)
        if not ini.has_section("config"):
            raise ValueError("the .ini of a LabSat 3 Wideband recording has no [config] section")
        cfg = ini["config"]
        qua = cfg.get("QUA") or cfg.get("QUAN_A")
        if not qua:
            raise ValueError("[config] has neither QUA nor QUAN_A")
        qua, chn = int(qua), int(cfg.get("CHN") or 0)
        if not 1 <= qua <= 3:
            raise ValueError(f"QUA {qua}: a sample quantization of 1, 2 or 3 bits is supported")
        if not 1 <= chn <= 3:
            raise ValueError(f"CHN {chn}: recordings of 1, 2 or 3 RF channels are supported")
        sft = 2 * qua * chn   # (a different SFT in the file is not valid: replaced, as the reference replaces it)
        sel = int(selected_channel)
        if not 1 <= sel <= chn:
            raise ValueError(f"selected_channel {sel}: the recording has {chn} RF channel(s)")
        f = cls(cls.LS3W_1BIT + qua - 1, cls.IQ, 8, rf_channels=chn, channel=sel - 1, flags=cls.DIGITAL_IO if digital_io_enabled else 0)
        assert f.samples_per_item * sft <= 64
        return f

    @classmethod
    def ls4(cls, qua: int, regs, channel: int = 0) -> "PackedFormat":
        """The LabSat 4 layout (QUA, regs): regs[s] 64-bit registers of channel slot s (A, B, C) per round, 0 for a slot that is not recorded; `channel`
        is the selected slot (0-based).  The register counts travel in big_endian_bytes, big_endian_items and flags (gsh_packed_format)."""
        if int(qua) not in cls.LS4_QUA:
            raise ValueError(f"QUA {qua}: a LabSat 4 sample quantization of 1, 2, 4, 8 or 12 bits is supported")
        regs = [int(r) for r in regs]
        if not 1 <= len(regs) <= 3:
            raise ValueError(f"{len(regs)} channel slots: a LabSat 4 layout describes 1 to 3 (A, B, C)")
        r = regs + [0] * (3 - len(regs))
        return cls(cls.LS4_QUA[int(qua)], cls.IQ, 8, r[0], r[1], rf_channels=len(regs), channel=channel, flags=r[2])

    @staticmethod
    def read_ls4_ini(text: str) -> dict:
        """The [config] and [channel X] entries of the .ini beside a LabSat 4 (.ls4) recording that the reference reads (read_ls3w_ini with d_is_ls4,
        gnuradio_blocks/labsat23_source.cc:700-920): QUA (else QUAN_A), CHN, SMP, BW_MAX, BW_DIV_A/B/C and BUF_SIZE_A/B/C -> dict(qua, chn, smp, bw_max,
        bw_div [3], buf_size [3]).  ValueError for a QUA outside 1, 2, 4, 8, 12 (:716), CHN above 3 (:761), a BUF_SIZE that is not a multiple of 8 (:846)
        and BUF_SIZE x BW_DIV that differ between the channels that have a buffer (:866-888)."""
        import configparser
        ini = configparser.ConfigParser(strict=False, interpolation=None)
        ini.optionxform = str
        ini.read_string(text)
        if not ini.has_section("config"):
            raise ValueError("the .ini of a LabSat 4 recording has no [config] section")
        cfg = ini["config"]
        qua = cfg.get("QUA") or cfg.get("QUAN_A")
        if not qua:
            raise ValueError("[config] has neither QUA nor QUAN_A")
        qua, chn = int(qua), int(cfg.get("CHN") or 0)
        if qua not in PackedFormat.LS4_QUA:
            raise ValueError(f"QUA {qua}: a LabSat 4 sample quantization of 1, 2, 4, 8 or 12 bits is supported")
        if not 1 <= chn <= 3:
            raise ValueError(f"CHN {chn}: recordings of 1, 2 or 3 RF channels are supported")
        bw_div, buf = [], []
        for x in "ABC":
            bw_div.append(int(cfg.get("BW_DIV_" + x) or 1))   # (the reference's default divisor is 1)
            size = int(ini[f"channel {x}"].get("BUF_SIZE_" + x) or 0) if ini.has_section(f"channel {x}") else 0
            if size > 0 and size % 8:
                raise ValueError(f"BUF_SIZE_{x} {size} is not a multiple of 8")
            buf.append(max(size, 0))
        relative = {b * d for b, d in zip(buf, bw_div) if b * d > 0}   # (are_equal_ignore_nonpositive)
        if len(relative) > 1:
            raise ValueError(f"BUF_SIZE x BW_DIV differs between the channels ({', '.join(f'{b} x {d}' for b, d in zip(buf, bw_div) if b > 0)}): "
                             "the buffer size configuration is invalid")
        return dict(qua=qua, chn=chn, smp=float(cfg.get("SMP") or 0), bw_max=int(cfg.get("BW_MAX") or 0), bw_div=bw_div, buf_size=buf)

    @classmethod
    def from_ls4_ini(cls, text: str, selected_channel: int = 1) -> "PackedFormat":
        """The format of a LabSat 4 (.ls4) recording from the text of the .ini beside it (read_ls4_ini).  regs[s] = BUF_SIZE_s / 8 for the three slots;
        the single-channel calls take slot selected_channel - 1, which must lie within CHN (:932) and have a buffer."""
        cfg = cls.read_ls4_ini(text)
        sel = int(selected_channel)
        if not 1 <= sel <= cfg["chn"]:
            raise ValueError(f"selected_channel {sel}: the recording has {cfg['chn']} RF channel(s)")
        if cfg["buf_size"][sel - 1] == 0:
            raise ValueError(f"selected_channel {sel}: channel {'ABC'[sel - 1]} has no BUF_SIZE_{'ABC'[sel - 1]} in the .ini: it is not recorded")
        return cls.ls4(cfg["qua"], [b // 8 for b in cfg["buf_size"]], sel - 1)

    @property
    def is_ls4(self) -> bool:
        return self.LS4_1BIT <= self.family <= self.LS4_12BIT

    @property
    def ls4_qua(self) -> int:
        return {v: k for k, v in self.LS4_QUA.items()}[self.family]

    @property
    def ls4_regs(self) -> "tuple[int, int, int]":
        """registers of slots A, B, C per round of a LabSat 4 layout"""
        return (self.big_endian_bytes, self.big_endian_items, self.flags)

    @property
    def ls4_round_bytes(self) -> int:
        return 8 * sum(self.ls4_regs)

    def ls4_samples_per_round(self, channel: int | None = None) -> int:
        """samples of slot `channel` (default: the selected one) in one round: regs x 32 / QUA"""
        return self.ls4_regs[self.channel if channel is None else channel] * 32 // self.ls4_qua

    def with_channel(self, channel: int) -> "PackedFormat":
        return PackedFormat(self.family, self.sample_type, self.item_size, self.big_endian_bytes, self.big_endian_items, self.rf_channels, channel,
                            self.flags)

    @property
    def is_register_family(self) -> bool:
        return self.LABSAT_2BIT <= self.family <= self.SPIR_1BIT or self.is_ls4

    @property
    def is_complex(self) -> bool:
        return (self.family in (self.TWO_BIT_CPX, self.FOUR_BIT_CPX, self.GSS6450_2BIT, self.GSS6450_4BIT) or self.is_register_family
                or (self.family == self.TWO_BIT and self.sample_type != self.REAL))

    @property
    def samples_per_byte(self) -> int:
        """samples of one RF channel per packed byte (GSS6450: per byte of the channel's own words).  Not meaningful for the register families, whose
        fields straddle bytes: samples_per_item / item_bytes"""
        if self.is_register_family:
            raise ValueError(f"packed family {self.family} has no whole number of samples per byte: use samples_per_item / item_bytes")
        if self.family == self.TWO_BIT:
            return 2 if self.is_complex else 4
        return {self.TWO_BIT_CPX: 2, self.FOUR_BIT_CPX: 1, self.NSR: 4, self.NTLAB: 1, self.GSS6450_2BIT: 2, self.GSS6450_4BIT: 1}[self.family]

    @property
    def item_bytes(self) -> int:
        """bytes of one input item: the 64-bit register of LS3W, the 16-bit item of LabSat 2 / 3, the 32-bit item of SPIR and word of GSS6450, the byte or
        short of the other families.  LabSat 4 at QUA 12: the 24 bytes of a triple of registers, which hold samples_per_item = 8 whole samples"""
        if self.family == self.LS4_12BIT:
            return 24
        return self.item_size

    @property
    def samples_per_item(self) -> int:
        """samples of one RF channel in one input item (LS3W: in one register, which holds as many of every RF channel; LS4: in one register of a
        slot's buffer, at QUA 12 in one triple of registers)"""
        if self.is_ls4:
            return 8 if self.family == self.LS4_12BIT else 32 // self.ls4_qua
        if self.LS3W_1BIT <= self.family <= self.LS3W_3BIT:
            return self.LS3W_SAMPLES_PER_REGISTER[(self.family - self.LS3W_1BIT + 1, self.rf_channels)][self.flags & self.DIGITAL_IO]
        if self.is_register_family:
            return {self.LABSAT_2BIT: 8, self.LABSAT_4BIT: 4, self.SPIR_1BIT: 1}[self.family]
        return self.samples_per_byte * self.item_size

    @property
    def interleaved_channels(self) -> int:
        """RF channels whose words share the packed stream (GSS6450 total_channels); 1 for every other family (the RF channels of LS3W share every
        register, not the stream item by item)"""
        return max(1, self.rf_channels) if self.family in (self.GSS6450_2BIT, self.GSS6450_4BIT) else 1

    def struct(self) -> "_lib.PackedFormat":
        return _lib.PackedFormat(self.family, self.sample_type, self.item_size, self.big_endian_bytes, self.big_endian_items, self.rf_channels,
                                 self.channel, self.flags)

    def __repr__(self):
        return (f"PackedFormat(family={self.family}, sample_type={self.sample_type}, item_size={self.item_size}, big_endian_bytes={self.big_endian_bytes}, "
                f"big_endian_items={self.big_endian_items}, rf_channels={self.rf_channels}, channel={self.channel}, flags={self.flags})")


def packed_bytes(fmt: PackedFormat, n_samples: int) -> int:
    """gsh_packed_bytes: bytes that hold n_samples samples per RF channel (GshError for a bad format or a partial input item).  No GPU."""
    out = C.c_uint64(0)
    f = fmt.struct()
    check(_lib.load().gsh_packed_bytes(C.byref(f), int(n_samples), C.byref(out)))
    return int(out.value)


def unpack_device(device: int, fmt: PackedFormat, src_ptr: int, first_sample: int, n_samples: int, dst_ptr: int, inverted_spectrum: bool = False,
                  hip_stream: int = 0) -> None:
    """gsh_unpack_device: complex64 (complex families) or float32 of fmt.channel (real families) for samples [first_sample, first_sample + n) of a
    device-resident packed buffer."""
    f = fmt.struct()
    check(_lib.load().gsh_unpack_device(device, C.byref(f), C.c_void_p(src_ptr), int(first_sample), int(n_samples), int(inverted_spectrum),
                                        C.c_void_p(dst_ptr), C.c_void_p(hip_stream) if hip_stream else None))


def _packed_host(fmt: PackedFormat, data, n_samples):
    a = np.ascontiguousarray(np.frombuffer(data, np.uint8) if isinstance(data, (bytes, bytearray)) else data).view(np.uint8).reshape(-1)
    if n_samples is not None:
        return a, int(n_samples)
    if fmt.is_ls4:   # whole rounds of the selected slot
        return a, a.size // fmt.ls4_round_bytes * fmt.ls4_samples_per_round()
    if fmt.is_register_family:
        return a, a.size // fmt.item_bytes * fmt.samples_per_item
    n = a.size * fmt.samples_per_byte // fmt.interleaved_channels
    return a, n


def packed_decode_host(fmt: PackedFormat, data, first_sample: int, n_samples: int) -> np.ndarray:
    """gsh_packed_decode_host: the host build of the decoder every device path shares -> complex64 [n_samples] of fmt.channel.  No GPU."""
    a = np.ascontiguousarray(data).view(np.uint8).reshape(-1)
    out = np.empty(int(n_samples), np.complex64)
    f = fmt.struct()
    check(_lib.load().gsh_packed_decode_host(C.byref(f), C.c_void_p(a.ctypes.data), int(first_sample), int(n_samples), fptr(out.view(np.float32))))
    return out


def unpack_device_multi(device: int, fmt: PackedFormat, src_ptr: int, first_sample: int, n_samples: int, channels, dst_ptrs,
                        inverted_spectrum: bool = False, hip_stream: int = 0) -> None:
    """gsh_unpack_device_multi: complex64 samples [first_sample, first_sample + n) of band channels[i] of a device-resident multi-band packed
    block -> dst_ptrs[i], every band in one pass over the block."""
    f = fmt.struct()
    ch = (C.c_int32 * len(channels))(*[int(c) for c in channels])
    dst = (C.c_void_p * len(dst_ptrs))(*[int(p) for p in dst_ptrs])
    check(_lib.load().gsh_unpack_device_multi(device, C.byref(f), C.c_void_p(src_ptr), int(first_sample), int(n_samples), int(inverted_spectrum),
                                              ch, len(channels), dst, C.c_void_p(hip_stream) if hip_stream else None))


def _multi_args(rings, channels):
    if len(rings) != len(channels):
        raise ValueError(f"{len(rings)} rings for {len(channels)} channels")
    return (C.c_void_p * len(rings))(*[r._h.value for r in rings]), (C.c_int32 * len(channels))(*[int(c) for c in channels]), (C.c_uint64 * max(1, len(rings)))()


def push_packed_multi(rings, channels, fmt: PackedFormat, data, inverted_spectrum: bool = False, n_samples: int | None = None) -> list[int]:
    """gsh_stream_push_packed_multi: one multi-band packed block held in host memory, band channels[i] into rings[i]; synchronous.  Returns the absolute
    index of the first sample in every ring."""
    a, n = _packed_host(fmt, data, n_samples)
    h, ch, first = _multi_args(rings, channels)
    f = fmt.struct()
    check(_lib.load().gsh_stream_push_packed_multi(h, ch, len(rings), C.byref(f), C.c_void_p(a.ctypes.data) if a.size else None, n, int(inverted_spectrum),
                                                   first))
    return [int(first[i]) for i in range(len(rings))]


def push_packed_multi_device(rings, channels, fmt: PackedFormat, device_ptr: int, n_samples: int, inverted_spectrum: bool = False,
                             hip_stream: int = 0) -> list[int]:
    h, ch, first = _multi_args(rings, channels)
    f = fmt.struct()
    check(_lib.load().gsh_stream_push_packed_multi_device(h, ch, len(rings), C.byref(f), C.c_void_p(device_ptr), int(n_samples), int(inverted_spectrum),
                                                          C.c_void_p(hip_stream) if hip_stream else None, first))
    return [int(first[i]) for i in range(len(rings))]


def push_packed_multi_pinned_async(rings, channels, fmt: PackedFormat, data: np.ndarray, inverted_spectrum: bool = False,
                                   n_samples: int | None = None) -> list[int]:
    """gsh_stream_push_packed_multi_pinned_async: `data` lies in page-locked memory and must stay untouched until wait_copied() / wait_copied_upto()
    on any ring of the call covers the push; nothing waits here."""
    a, n = _packed_host(fmt, data, n_samples)
    h, ch, first = _multi_args(rings, channels)
    f = fmt.struct()
    check(_lib.load().gsh_stream_push_packed_multi_pinned_async(h, ch, len(rings), C.byref(f), C.c_void_p(a.ctypes.data) if a.size else None, n,
                                                                int(inverted_spectrum), first))
    return [int(first[i]) for i in range(len(rings))]


class SampleStream:
    def __init__(self, capacity_samples: int, max_window_samples: int, device: int = 0):
        self._lib = _lib.load()
        self._h = C.c_void_p()
        self.device = device
        check(self._lib.gsh_stream_create(device, capacity_samples, max_window_samples, C.byref(self._h)))

    def close(self):
        if self._h and getattr(self, "_owned", True):
            self._lib.gsh_stream_destroy(self._h)
        self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def push(self, items: np.ndarray, item_type: str = "gr_complex", inverted_spectrum: bool = False) -> int:
        """Append samples held in host memory (complex64 [n], or int16 / int8 [n, 2] interleaved I,Q).  Returns the absolute
        index of the first one."""
        t = ITEM_TYPES[item_type]
        items = np.asarray(items)
        if t == GSH_ITEM_GR_COMPLEX and not np.iscomplexobj(items):
            items = np.ascontiguousarray(items, np.float32).reshape(-1).view(np.complex64)   # interleaved float32 I,Q as read from a file
        a = np.ascontiguousarray(items, _NP[t])
        n = a.size if t == GSH_ITEM_GR_COMPLEX else a.size // 2
        first = C.c_uint64(0)
        check(self._lib.gsh_stream_push(self._h, C.c_void_p(a.ctypes.data), n, t, int(inverted_spectrum), C.byref(first)))
        return int(first.value)

    def push_device(self, device_ptr: int, n: int, item_type: str = "gr_complex", inverted_spectrum: bool = False, hip_stream: int = 0) -> int:
        first = C.c_uint64(0)
        check(self._lib.gsh_stream_push_device(self._h, C.c_void_p(device_ptr), n, ITEM_TYPES[item_type], int(inverted_spectrum),
                                               C.c_void_p(hip_stream) if hip_stream else None, C.byref(first)))
        return int(first.value)

    def push_async(self, items: np.ndarray, item_type: str = "gr_complex", inverted_spectrum: bool = False) -> int:
        """gsh_stream_push_async: copy + conversion queued on the ring's stream, returns at once.  `items` (numpy array, or a host pointer
        given as (ptr, n)) must stay untouched until wait() or two further pushes."""
        first = C.c_uint64(0)
        if isinstance(items, tuple):
            ptr, n = items
        else:
            ptr, n = items.ctypes.data, (items.size // 2 if item_type != "gr_complex" or items.dtype != np.complex64 else items.size)
            self._keep_async = getattr(self, "_keep_async", [])[-2:] + [items]
        check(self._lib.gsh_stream_push_async(self._h, C.c_void_p(ptr), n, ITEM_TYPES[item_type], int(inverted_spectrum), C.byref(first)))
        return int(first.value)

    def push_staged(self, items: np.ndarray, item_type: str = "gr_complex", inverted_spectrum: bool = False) -> int:
        """gsh_stream_push_staged: `items` (any host memory) is copied into the ring's page-locked staging on the spot, so the array is free on
        return; the DMA and the conversion are queued, nothing waits but for the push that used the staging pair four pushes ago."""
        t = ITEM_TYPES[item_type]
        a = np.ascontiguousarray(items, _NP[t])
        n = a.size if t == GSH_ITEM_GR_COMPLEX else a.size // 2
        first = C.c_uint64(0)
        check(self._lib.gsh_stream_push_staged(self._h, C.c_void_p(a.ctypes.data) if n else None, n, t, int(inverted_spectrum), C.byref(first)))
        return int(first.value)

    def push_pinned_async(self, items: np.ndarray, item_type: str = "gr_complex", inverted_spectrum: bool = False) -> int:
        """gsh_stream_push_pinned_async: `items` lies in page-locked memory (gsh_host_register) and must stay untouched until wait_copied() /
        wait_copied_upto() covers the push; the DMA and the conversion are queued, nothing waits."""
        t = ITEM_TYPES[item_type]
        a = np.ascontiguousarray(items, _NP[t])
        n = a.size if t == GSH_ITEM_GR_COMPLEX else a.size // 2
        self._keep_async = getattr(self, "_keep_async", [])[-3:] + [a]
        first = C.c_uint64(0)
        check(self._lib.gsh_stream_push_pinned_async(self._h, C.c_void_p(a.ctypes.data) if n else None, n, t, int(inverted_spectrum), C.byref(first)))
        return int(first.value)

    def push_pinned(self, items: np.ndarray, item_type: str = "gr_complex", inverted_spectrum: bool = False) -> int:
        """gsh_stream_push_pinned: `items` is page-locked for the call (gsh_host_register on its pages) and handed to the DMA engine as it lies --
        gr_complex items straight into their ring positions; returns when the array may be reused."""
        t = ITEM_TYPES[item_type]
        a = np.ascontiguousarray(items, _NP[t])
        n = a.size if t == GSH_ITEM_GR_COMPLEX else a.size // 2
        first = C.c_uint64(0)
        if n == 0:
            check(self._lib.gsh_stream_push_pinned(self._h, None, 0, t, int(inverted_spectrum), C.byref(first)))
            return int(first.value)
        lo = a.ctypes.data & ~4095
        hi = (a.ctypes.data + a.nbytes + 4095) & ~4095
        check(self._lib.gsh_host_register(self.device, C.c_void_p(lo), hi - lo))
        try:
            check(self._lib.gsh_stream_push_pinned(self._h, C.c_void_p(a.ctypes.data), n, t, int(inverted_spectrum), C.byref(first)))
        finally:
            check(self._lib.gsh_host_unregister(C.c_void_p(lo)))
        return int(first.value)

    def push_packed(self, fmt: PackedFormat, data, inverted_spectrum: bool = False, n_samples: int | None = None) -> int:
        """gsh_stream_push_packed: packed complex samples held in host memory (every sample of `data` unless n_samples says fewer); synchronous."""
        a, n = _packed_host(fmt, data, n_samples)
        f, first = fmt.struct(), C.c_uint64(0)
        check(self._lib.gsh_stream_push_packed(self._h, C.byref(f), C.c_void_p(a.ctypes.data) if a.size else None, n, int(inverted_spectrum), C.byref(first)))
        return int(first.value)

    def push_packed_device(self, fmt: PackedFormat, device_ptr: int, n_samples: int, inverted_spectrum: bool = False, hip_stream: int = 0) -> int:
        f, first = fmt.struct(), C.c_uint64(0)
        check(self._lib.gsh_stream_push_packed_device(self._h, C.byref(f), C.c_void_p(device_ptr), int(n_samples), int(inverted_spectrum),
                                                      C.c_void_p(hip_stream) if hip_stream else None, C.byref(first)))
        return int(first.value)

    def push_packed_pinned_async(self, fmt: PackedFormat, data: np.ndarray, inverted_spectrum: bool = False, n_samples: int | None = None) -> int:
        """gsh_stream_push_packed_pinned_async: `data` lies in page-locked memory (gsh_host_register) and must stay untouched until wait_copied() /
        wait_copied_upto() covers the push; the DMA and the unpack are queued, nothing waits."""
        a, n = _packed_host(fmt, data, n_samples)
        self._keep_async = getattr(self, "_keep_async", [])[-3:] + [a]
        f, first = fmt.struct(), C.c_uint64(0)
        check(self._lib.gsh_stream_push_packed_pinned_async(self._h, C.byref(f), C.c_void_p(a.ctypes.data) if a.size else None, n, int(inverted_spectrum),
                                                            C.byref(first)))
        return int(first.value)

    def wait_copied(self) -> None:
        check(self._lib.gsh_stream_wait_copied(self._h))

    def wait_copied_upto(self, end_index: int) -> int:
        """blocks until every push that covers samples below end_index has been read out of the caller's memory; returns the index up to which the
        ring is known to be complete"""
        upto = C.c_uint64(0)
        check(self._lib.gsh_stream_wait_copied_upto(self._h, int(end_index), C.byref(upto)))
        return int(upto.value)

    def wait(self) -> None:
        check(self._lib.gsh_stream_wait(self._h))

    def seek(self, next_index: int) -> None:
        check(self._lib.gsh_stream_seek(self._h, int(next_index)))

    def range(self):
        lo, hi = C.c_uint64(0), C.c_uint64(0)
        check(self._lib.gsh_stream_range(self._h, C.byref(lo), C.byref(hi)))
        return int(lo.value), int(hi.value)

    def read(self, index: int, n: int) -> np.ndarray:
        out = np.empty(n, np.complex64)
        check(self._lib.gsh_stream_read(self._h, index, n, fptr(out)))
        return out


def convert_samples_device(device: int, src_ptr: int, item_type: str, dst_ptr: int, n: int, inverted_spectrum: bool = False, hip_stream: int = 0) -> None:
    check(_lib.load().gsh_convert_samples_device(device, C.c_void_p(src_ptr), ITEM_TYPES[item_type], int(inverted_spectrum), C.c_void_p(dst_ptr), n,
                                                 C.c_void_p(hip_stream) if hip_stream else None))


def direct_resample_device(device: int, src_ptr: int, in0: int, n_in: int, fs_in: float, fs_out: float, out0: int, dst_ptr: int, max_out: int,
                           hip_stream: int = 0):
    """direct_resampler_conditioner_cc on the device (gsh_direct_resample_device).  -> (n_out, n_in_consumed)"""
    n_out, n_cons = C.c_uint64(0), C.c_uint64(0)
    check(_lib.load().gsh_direct_resample_device(device, C.c_void_p(src_ptr), in0, n_in, fs_in, fs_out, out0, C.c_void_p(dst_ptr), max_out,
                                                 C.byref(n_out), C.byref(n_cons), C.c_void_p(hip_stream) if hip_stream else None))
    return int(n_out.value), int(n_cons.value)


class FirFilter:
    """gsh_fir_*: frequency-translating decimating FIR filter with stream history (freq_xlating_fir_filter_ccf / fir_filter_ccf on the device)."""
    KINDS = {"gr_complex": 0, "float": 1, "short": 2, "byte": 3}

    def __init__(self, taps, decimation: int = 1, center_freq_hz: float = 0.0, sampling_freq_hz: float = 1.0, input_kind="gr_complex", device: int = 0):
        """input_kind: "gr_complex", "float", "short", "byte", or a PackedFormat (gsh_fir_create_packed: process_device then reads packed bytes, n_in
        counting samples of the format's RF channel)."""
        self._lib = _lib.load()
        self._h = C.c_void_p()
        t = np.ascontiguousarray(taps, np.float32)
        self.decimation = decimation
        if isinstance(input_kind, PackedFormat):
            f = input_kind.struct()
            check(self._lib.gsh_fir_create_packed(device, fptr(t), len(t), decimation, center_freq_hz, sampling_freq_hz, C.byref(f), C.byref(self._h)))
        else:
            check(self._lib.gsh_fir_create(device, fptr(t), len(t), decimation, center_freq_hz, sampling_freq_hz, self.KINDS[input_kind], C.byref(self._h)))

    def close(self):
        if self._h:
            self._lib.gsh_fir_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def process_device(self, in_ptr: int, n_in: int, out_ptr: int, max_out: int, hip_stream: int = 0) -> int:
        n_out = C.c_uint64(0)
        check(self._lib.gsh_fir_process_device(self._h, C.c_void_p(in_ptr), n_in, C.c_void_p(out_ptr), max_out, C.byref(n_out),
                                               C.c_void_p(hip_stream) if hip_stream else None))
        return int(n_out.value)


def firdes_low_pass(gain: float, sampling_freq: float, cutoff_freq: float, transition_width: float) -> np.ndarray:
    """gr::filter::firdes::low_pass with the default Hamming window, as restated in host/hip_acq_resampler.h (GNU Radio is not
    vendored: published algorithm, parity unpinned)."""
    ntaps = int(53.0 * sampling_freq / (22.0 * transition_width))
    if ntaps % 2 == 0:
        ntaps += 1
    n = np.arange(ntaps)
    w = (0.54 - 0.46 * np.cos(2.0 * np.pi * n / (ntaps - 1))).astype(np.float32)
    m = (ntaps - 1) // 2
    k = n - m
    fw = 2.0 * np.pi * cutoff_freq / sampling_freq
    with np.errstate(invalid="ignore", divide="ignore"):
        taps = np.where(k == 0, fw / np.pi, np.sin(k * fw) / (k * np.pi)) * w
    taps = taps.astype(np.float32)
    fmax = float(taps[m]) + 2.0 * float(np.sum(taps[m + 1:].astype(np.float64)))
    return (taps.astype(np.float64) * (gain / fmax)).astype(np.float32)


def acquisition_resampler_design(fs: int, acq_fs: float):
    """(decimation, decimated rate, taps, latency) as GNSSFlowgraph sets the acquisition resampler up (gnss_flowgraph.cc:1165-1211)."""
    if not acq_fs < fs:
        return 1, float(fs), np.zeros(0, np.float32), 0
    decimation = int(np.floor(fs / acq_fs))
    while fs % decimation > 0:
        decimation -= 1
    if decimation <= 1:
        return 1, float(fs), np.zeros(0, np.float32), 0
    dec_fs = fs / decimation
    taps = firdes_low_pass(1.0, fs, dec_fs / 2.1, dec_fs / 2)
    return decimation, dec_fs, taps, (len(taps) - 1) // 2


class PulseBlanking:
    """gsh_pb_*: pulse_blanking_cc on the device (pulse_blanking_cc.cc:33-106)."""

    def __init__(self, pfa: float = 0.04, length: int = 32, n_segments_est: int = 12500, n_segments_reset: int = 5000000, device: int = 0):
        self._lib = _lib.load()
        self._h = C.c_void_p()
        check(self._lib.gsh_pb_create(device, pfa, length, n_segments_est, n_segments_reset, C.byref(self._h)))
        self.length = length

    def close(self):
        if self._h:
            self._lib.gsh_pb_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def threshold(self) -> float:
        return float(self._lib.gsh_pb_threshold(self._h))

    def process_device(self, d_in: int, n_items: int, d_out: int) -> int:
        """One general_work call over n_items resident samples; returns how many were consumed (= produced)."""
        done = C.c_uint64(0)
        check(self._lib.gsh_pb_process_device(self._h, C.c_void_p(d_in), n_items, C.c_void_p(d_out), C.byref(done)))
        return int(done.value)

    def state(self):
        noise, n, last = C.c_float(0.0), C.c_int32(0), C.c_int32(0)
        check(self._lib.gsh_pb_get_state(self._h, C.byref(noise), C.byref(n), C.byref(last)))
        return float(noise.value), int(n.value), bool(last.value)


class NotchFilter:
    """gsh_notch_*: Notch (notch_cc.cc:33-140; n_segments_coeff = 0) or NotchLite (notch_lite_cc.cc:30-150; n_segments_coeff >= 1) on the device."""

    def __init__(self, pfa: float = 0.001, p_c_factor: float = 0.9, length: int = 32, n_segments_est: int = 12500, n_segments_reset: int = 5000000,
                 n_segments_coeff: int = 0, device: int = 0):
        self._lib = _lib.load()
        self._h = C.c_void_p()
        check(self._lib.gsh_notch_create(device, pfa, p_c_factor, length, n_segments_est, n_segments_reset, n_segments_coeff, C.byref(self._h)))
        self.length = length

    def close(self):
        if self._h:
            self._lib.gsh_notch_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def threshold(self) -> float:
        return float(self._lib.gsh_notch_threshold(self._h))

    def process_device(self, d_in: int, n_items: int, d_out: int) -> int:
        """One general_work call over n_items resident items (item 0: the sample in front of the first one processed); returns how many were
        consumed (= produced; out[k] is the filtered in[k + 1])."""
        done = C.c_uint64(0)
        check(self._lib.gsh_notch_process_device(self._h, C.c_void_p(d_in), n_items, C.c_void_p(d_out), C.byref(done)))
        return int(done.value)

    def state(self) -> dict:
        noise, n, fs, nc = C.c_float(0.0), C.c_int32(0), C.c_int32(0), C.c_int32(0)
        lo, z0 = (C.c_float * 2)(), (C.c_float * 2)()
        check(self._lib.gsh_notch_get_state(self._h, C.byref(noise), C.byref(n), C.byref(fs), lo, C.byref(nc), z0))
        return dict(noise_pow_est=float(noise.value), n_segments=int(n.value), filter_state=bool(fs.value), last_out=complex(lo[0], lo[1]),
                    n_segments_coeff=int(nc.value), z0=complex(z0[0], z0[1]))


class StreamGroup:
    """gsh_stream_group_*: one block replicated into the sample rings of several GPUs over RCCL (one process per GPU: from_rank; one process
    driving several GPUs: local)."""
    MODES = {"broadcast": 0, "scatter_allgather": 1}
    FORCE_RCCL = 0x100   # GSH_GROUP_FORCE_RCCL: a group of one builds its communicator and runs the mode's collectives all the same

    def __init__(self, handle, lib):
        self._h, self._lib = handle, lib

    @staticmethod
    def unique_id() -> bytes:
        buf = C.create_string_buffer(128)
        check(_lib.load().gsh_comm_unique_id(buf))
        return buf.raw

    class _Op(C.Structure):
        _fields_ = [("op", C.c_int32), ("peer", C.c_int32), ("phase", C.c_int32), ("src_buf", C.c_int32), ("dst_buf", C.c_int32),
                    ("src_offset", C.c_uint64), ("dst_offset", C.c_uint64), ("bytes", C.c_uint64)]

    OPS = {0: "broadcast", 1: "send", 2: "recv", 3: "allgather"}
    BUFS = {0: None, 1: "stage", 2: "piece"}

    @classmethod
    def plan(cls, nbytes: int, world: int, rank: int, mode: str = "broadcast"):
        """gsh_stream_group_plan: (padded_bytes, [dict(op, peer, phase, src_buf, dst_buf, src_offset, dst_offset, bytes)]) -- the operations a push of
        `nbytes` raw bytes issues on `rank`, the list the engine itself walks.  Needs no GPU."""
        L = _lib.load()
        n, padded = C.c_int(0), C.c_uint64(0)
        check(L.gsh_stream_group_plan(nbytes, world, rank, cls.MODES[mode], None, 0, C.byref(n), C.byref(padded)))
        ops = (cls._Op * max(n.value, 1))()
        check(L.gsh_stream_group_plan(nbytes, world, rank, cls.MODES[mode], ops, n.value, C.byref(n), C.byref(padded)))
        return int(padded.value), [dict(op=cls.OPS[o.op], peer=int(o.peer), phase=int(o.phase), src_buf=cls.BUFS[o.src_buf], dst_buf=cls.BUFS[o.dst_buf],
                                        src_offset=int(o.src_offset), dst_offset=int(o.dst_offset), bytes=int(o.bytes)) for o in ops[:n.value]]

    @staticmethod
    def library() -> str:
        """File name of the collective library the engine has loaded (gsh_comm_library): the system's librccl, or what GSH_RCCL_LIBRARY names."""
        buf = C.create_string_buffer(1024)
        check(_lib.load().gsh_comm_library(buf, 1024))
        return buf.value.decode()

    @classmethod
    def from_rank(cls, device: int, rank: int, world: int, unique_id: bytes | None, capacity_samples: int, max_window_samples: int, mode: str = "broadcast",
                  force_rccl: bool = False):
        L = _lib.load()
        h = C.c_void_p()
        idb = C.create_string_buffer(unique_id, 128) if unique_id is not None else None
        check(L.gsh_stream_group_create_rank(device, rank, world, idb, capacity_samples, max_window_samples,
                                             cls.MODES[mode] | (cls.FORCE_RCCL if force_rccl else 0), C.byref(h)))
        return cls(h, L)

    @classmethod
    def local(cls, devices, capacity_samples: int, max_window_samples: int, mode: str = "broadcast", force_rccl: bool = False):
        L = _lib.load()
        h = C.c_void_p()
        arr = (C.c_int * len(devices))(*devices)
        check(L.gsh_stream_group_create(arr, len(devices), capacity_samples, max_window_samples,
                                        cls.MODES[mode] | (cls.FORCE_RCCL if force_rccl else 0), C.byref(h)))
        return cls(h, L)

    def rccl_info(self) -> dict:
        """{'ranks': ranks of the communicator the group built (0: RCCL untouched), 'version': ncclGetVersion code, 'collectives': RCCL calls issued}"""
        ranks, ver, calls = C.c_int32(0), C.c_int32(0), C.c_uint64(0)
        check(self._lib.gsh_stream_group_rccl_info(self._h, C.byref(ranks), C.byref(ver), C.byref(calls)))
        return dict(ranks=int(ranks.value), version=int(ver.value), collectives=int(calls.value))

    def close(self):
        if self._h:
            self._lib.gsh_stream_group_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def size(self) -> int:
        return self._lib.gsh_stream_group_size(self._h)

    def ring(self, local_index: int = 0) -> "SampleStream":
        """The group's ring as a SampleStream view (owned by the group: closing the view does nothing)."""
        s = SampleStream.__new__(SampleStream)
        s._lib = self._lib
        s._h = C.c_void_p(self._lib.gsh_stream_group_ring(self._h, local_index))
        s._owned = False
        s._group = self
        return s

    def push_device(self, device_ptr: int | None, n: int, item_type: str = "ibyte", inverted_spectrum: bool = False) -> int:
        first = C.c_uint64(0)
        check(self._lib.gsh_stream_group_push_device(self._h, C.c_void_p(device_ptr) if device_ptr else None, n, ITEM_TYPES[item_type],
                                                     int(inverted_spectrum), C.byref(first)))
        return int(first.value)

    def push(self, items: np.ndarray | None, n: int, item_type: str = "ibyte", inverted_spectrum: bool = False) -> int:
        first = C.c_uint64(0)
        ptr = C.c_void_p(items.ctypes.data) if items is not None else None
        check(self._lib.gsh_stream_group_push(self._h, ptr, n, ITEM_TYPES[item_type], int(inverted_spectrum), C.byref(first)))
        return int(first.value)

    def push_packed(self, fmt: PackedFormat, data, n_samples: int | None = None, inverted_spectrum: bool = False) -> int:
        """gsh_stream_group_push_packed: every rank calls it; rank 0's process supplies the packed bytes, the others pass data = None and n_samples"""
        f, first = fmt.struct(), C.c_uint64(0)
        if data is None:
            ptr, n = None, int(n_samples)
        else:
            a, n = _packed_host(fmt, data, n_samples)
            ptr = C.c_void_p(a.ctypes.data) if a.size else None
        check(self._lib.gsh_stream_group_push_packed(self._h, C.byref(f), ptr, n, int(inverted_spectrum), C.byref(first)))
        return int(first.value)

    def push_packed_device(self, fmt: PackedFormat, device_ptr: int | None, n_samples: int, inverted_spectrum: bool = False) -> int:
        f, first = fmt.struct(), C.c_uint64(0)
        check(self._lib.gsh_stream_group_push_packed_device(self._h, C.byref(f), C.c_void_p(device_ptr) if device_ptr else None, int(n_samples),
                                                            int(inverted_spectrum), C.byref(first)))
        return int(first.value)

    def wait(self) -> None:
        check(self._lib.gsh_stream_group_wait(self._h))
