"""ION GNSS SDR metadata standard (ION_GSMS) recordings: the layout object behind gsh_ion_* (include/gnss_sdr_hip.h has the bit stream, the values and
the deviations from the reference), a reader of the metadata XML and a reader of the recording that hands whole cycles to the device.

Stands in for ION_GSMS_Signal_Source (adapters/ion_gsms_signal_source.cc, gnuradio_blocks/ion_gsms.cc, libs/ion_gsms_chunk_data.cc)."""
from __future__ import annotations

import ctypes as C
import os
import re
import xml.etree.ElementTree as ET

import numpy as np

from . import _lib
from ._lib import IonChunk, IonStream, check, fptr

ENCODINGS = {"SIGN": 0, "OB": 1, "SM": 2, "MS": 3, "TC": 4, "OG": 5, "OBA": 6, "SMA": 7, "MSA": 8, "TCA": 9, "OGA": 10, "FP": 11}
REAL, IQ, QI = 0, 1, 2
_FORMATS = {"real": REAL, "if": REAL, "iq": IQ, "qi": QI}
_ALIGN = {"undefined": 0, "left": 1, "right": 2}
_SHIFT = {"undefined": 0, "left": 0, "right": 1}


def _enum(value, names, what):
    if isinstance(value, str):
        if value.strip().lower() not in names:
            raise ValueError(f"unknown {what} {value!r}")
        return names[value.strip().lower()]
    return int(value)


def parse_format(text: str) -> tuple[int, int]:
    """a format of the standard (IF, IFn, IQ, IQn, InQ, InQn, QI, QIn, QnI, QnIn) -> (GSH_PACKED_REAL / _IQ / _QI, negate): an `n` behind a
    component negates it; negate bit 0 is I (or the real value), bit 1 is Q"""
    t = text.strip()
    m = re.fullmatch(r"(?i)if(n?)", t)
    if m:
        return REAL, 1 if m.group(1) else 0
    m = re.fullmatch(r"(?i)([iq])(n?)([iq])(n?)", t)
    if not m or m.group(1).lower() == m.group(3).lower():
        raise ValueError(f"unknown stream format {text!r}")
    first_i = m.group(1).lower() == "i"
    neg_first, neg_second = bool(m.group(2)), bool(m.group(4))
    neg_i, neg_q = (neg_first, neg_second) if first_i else (neg_second, neg_first)
    return (IQ if first_i else QI), int(neg_i) | int(neg_q) << 1


class IonLayout:
    """gsh_ion_layout_t.  `chunks`: one mapping per chunk of the cycle with the fields of gsh_ion_chunk (size_word, count_words, big_endian, shift,
    padding, n_streams); `streams`: the streams of every chunk in order, mappings with the fields of gsh_ion_stream (packed_bits, rate_factor,
    quantization, encoding, format, alignment, lump_shift, negate) and an optional `name`.  encoding, format, alignment and the shifts may be given by
    name ("TC", "qi", "left", "right").  Streams are selected by index or by name."""

    def __init__(self, chunks, streams):
        self._lib = _lib.load()
        self._h = C.c_void_p()
        self.names = [s.get("name") for s in streams]
        cs = (IonChunk * max(1, len(chunks)))()
        for o, c in zip(cs, chunks):
            o.size_word, o.count_words, o.n_streams = int(c["size_word"]), int(c["count_words"]), int(c["n_streams"])
            o.big_endian = int(c.get("big_endian", 0))
            o.shift = _enum(c.get("shift", 0), _SHIFT, "word shift")
            o.padding = _enum(c.get("padding", 0), {"none": 0, "tail": 0, "head": 1}, "padding")
        ss = (IonStream * max(1, len(streams)))()
        for o, s in zip(ss, streams):
            o.packed_bits, o.rate_factor, o.quantization = int(s["packed_bits"]), int(s["rate_factor"]), int(s["quantization"])
            o.encoding = _enum(s["encoding"], {k.lower(): v for k, v in ENCODINGS.items()}, "encoding")
            o.format = _enum(s.get("format", REAL), _FORMATS, "format")
            o.alignment = _enum(s.get("alignment", 0), _ALIGN, "alignment")
            o.lump_shift = _enum(s.get("lump_shift", 0), _SHIFT, "lump shift")
            o.negate = int(s.get("negate", 0))
        check(self._lib.gsh_ion_layout_create(cs, len(chunks), ss, len(streams), C.byref(self._h)))
        cb, ns = C.c_uint32(), C.c_int32()
        check(self._lib.gsh_ion_layout_info(self._h, C.byref(cb), C.byref(ns)))
        self.cycle_bytes, self.n_streams = int(cb.value), int(ns.value)

    def close(self) -> None:
        if getattr(self, "_h", None):
            self._lib.gsh_ion_layout_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def index(self, stream) -> int:
        if isinstance(stream, str):
            if stream not in self.names:
                raise KeyError(f"no stream named {stream!r}")
            return self.names.index(stream)
        return int(stream)

    def _indices(self, streams):
        idx = [self.index(s) for s in streams]
        return idx, (C.c_int32 * max(1, len(idx)))(*idx)

    def stream_info(self, stream) -> tuple[int, bool, int]:
        """(samples per cycle, complex?, bits of a field)"""
        spc, cplx, w = C.c_int32(), C.c_int32(), C.c_int32()
        check(self._lib.gsh_ion_stream_info(self._h, self.index(stream), C.byref(spc), C.byref(cplx), C.byref(w)))
        return int(spc.value), bool(cplx.value), int(w.value)

    def bytes_for(self, stream, n_samples: int) -> int:
        """bytes of the cycles that samples [0, n_samples) of the stream touch"""
        b = C.c_uint64()
        check(self._lib.gsh_ion_bytes(self._h, self.index(stream), int(n_samples), C.byref(b)))
        return int(b.value)

    def decode_host(self, stream, data, first_sample: int = 0, n_samples: int | None = None) -> np.ndarray:
        """gsh_ion_decode_host: the host build of the kernel's decoder -> float32 (real stream) or complex64"""
        a = np.ascontiguousarray(data).view(np.uint8).reshape(-1)
        spc, cplx, _ = self.stream_info(stream)
        if n_samples is None:
            n_samples = a.size // self.cycle_bytes * spc - first_sample
        if n_samples < 0 or self.bytes_for(stream, first_sample + n_samples) > a.size:
            raise ValueError(f"samples [{first_sample}, {first_sample + n_samples}) lie outside a block of {a.size} bytes")
        out = np.empty(int(n_samples), np.complex64 if cplx else np.float32)
        check(self._lib.gsh_ion_decode_host(self._h, self.index(stream), C.c_void_p(a.ctypes.data) if a.size else None, int(first_sample), int(n_samples),
                                            fptr(out.view(np.float32))))
        return out

    def unpack_device(self, device: int, src_ptr: int, first_sample: int, n_samples: int, streams, dst_ptrs, inverted_spectrum: bool = False,
                      hip_stream: int = 0) -> None:
        """gsh_ion_unpack_device: one pass over the device-resident block writes every selected stream to its destination"""
        if len(dst_ptrs) != len(streams):
            raise ValueError(f"{len(dst_ptrs)} destinations for {len(streams)} streams")
        _, idx = self._indices(streams)
        dst = (C.c_void_p * max(1, len(dst_ptrs)))(*[int(p) for p in dst_ptrs])
        check(self._lib.gsh_ion_unpack_device(device, self._h, C.c_void_p(src_ptr), int(first_sample), int(n_samples), int(inverted_spectrum), idx,
                                              len(streams), dst, C.c_void_p(hip_stream) if hip_stream else None))

    def _push_args(self, rings, streams):
        if len(rings) != len(streams):
            raise ValueError(f"{len(rings)} rings for {len(streams)} streams")
        idx, arr = self._indices(streams)
        return (C.c_void_p * max(1, len(rings)))(*[r._h.value for r in rings]), idx, arr, (C.c_uint64 * max(1, len(rings)))()

    def _host_block(self, idx, data, n_samples):
        a = np.ascontiguousarray(data).view(np.uint8).reshape(-1)
        if n_samples is None:
            n_samples = a.size // self.cycle_bytes * self.stream_info(idx[0])[0] if idx else 0
        elif idx and self.bytes_for(idx[0], n_samples) > a.size:
            raise ValueError(f"{n_samples} samples need {self.bytes_for(idx[0], n_samples)} bytes, the block holds {a.size}")
        return a, int(n_samples)

    def push(self, rings, streams, data, inverted_spectrum: bool = False, n_samples: int | None = None) -> list[int]:
        """gsh_stream_push_ion: a block of whole cycles in host memory, complex stream streams[i] into rings[i]; synchronous.  Returns the absolute
        index of the first sample in every ring."""
        h, idx, arr, first = self._push_args(rings, streams)
        a, n = self._host_block(idx, data, n_samples)
        check(self._lib.gsh_stream_push_ion(h, arr, len(rings), self._h, C.c_void_p(a.ctypes.data) if a.size else None, n, int(inverted_spectrum), first))
        return [int(first[i]) for i in range(len(rings))]

    def push_device(self, rings, streams, device_ptr: int, n_samples: int, inverted_spectrum: bool = False, hip_stream: int = 0) -> list[int]:
        h, idx, arr, first = self._push_args(rings, streams)
        check(self._lib.gsh_stream_push_ion_device(h, arr, len(rings), self._h, C.c_void_p(device_ptr), int(n_samples), int(inverted_spectrum),
                                                   C.c_void_p(hip_stream) if hip_stream else None, first))
        return [int(first[i]) for i in range(len(rings))]

    def push_pinned_async(self, rings, streams, data: np.ndarray, inverted_spectrum: bool = False, n_samples: int | None = None) -> list[int]:
        """gsh_stream_push_ion_pinned_async: `data` lies in page-locked memory and must stay untouched until wait_copied() / wait_copied_upto() on any
        ring of the call covers the push; nothing waits here."""
        h, idx, arr, first = self._push_args(rings, streams)
        a, n = self._host_block(idx, data, n_samples)
        check(self._lib.gsh_stream_push_ion_pinned_async(h, arr, len(rings), self._h, C.c_void_p(a.ctypes.data) if a.size else None, n,
                                                         int(inverted_spectrum), first))
        return [int(first[i]) for i in range(len(rings))]


def _tag(el) -> str:
    return el.tag.rsplit("}", 1)[-1].lower()


class IonGsmsMetadata:
    """The part of an ION SDR metadata file (.sdrx) that the signal source reads: `file` (url, offset, lane), `lane`, `block` (cycles, sizeheader,
    sizefooter), `chunk` (sizeword, countwords, endian, padding, wordshift), `lump` (shift) and `stream` (ratefactor, quantization, packedbits,
    alignment, format, encoding).  An element without children that carries an `id` refers to the element of the same name and id defined elsewhere.
    Tags are matched case-insensitively and namespaces are ignored.  The GnssMetadata library is not available to check the element names against:
    they are the reference's accessor names (SizeWord, CountWords, Packedbits, RateFactor ...) in lower case.
    A stream without `format` gets the reference's inference: complex (IQ) when packedbits >= 2 ratefactor quantization (libs/ion_gsms_chunk_data.cc:60),
    else real.  A format with a negated component (IQn, InQ, QnI ...) sets `negate`.

    files: [{url, offset, lane}]; lanes: {id: [block]}; block: {cycles, sizeheader, sizefooter, chunks}; chunk and stream: the mappings IonLayout takes
    (a chunk carries its `streams`)."""

    def __init__(self, root):
        self._defs = {}
        for el in root.iter():
            if el.get("id") is not None and len(el):
                self._defs.setdefault((_tag(el), el.get("id")), el)
        self.files, self.lanes = [], {}
        for el in root.iter():
            if _tag(el) == "lane" and len(el):
                self.lanes.setdefault(el.get("id"), [self._block(b) for b in self._children(el, "block")])
        for el in root.iter():
            if _tag(el) == "file" and len(el):
                lane = self._children(el, "lane", resolve=False)
                self.files.append({"url": self._text(el, "url", ""), "offset": int(self._text(el, "offset", "0")),
                                   "lane": lane[0].get("id") if lane else None})

    @classmethod
    def parse(cls, path_or_text) -> "IonGsmsMetadata":
        text = str(path_or_text)
        if text.lstrip().startswith("<"):
            return cls(ET.fromstring(text))
        return cls(ET.parse(text).getroot())

    def _children(self, el, tag, resolve=True):
        out = []
        for c in el:
            if _tag(c) == tag:
                if resolve and not len(c) and c.get("id") is not None:
                    if (tag, c.get("id")) not in self._defs:
                        raise ValueError(f"<{tag} id={c.get('id')!r}> refers to an element that is not defined")
                    c = self._defs[(tag, c.get("id"))]
                out.append(c)
        return out

    @staticmethod
    def _text(el, tag, default=None):
        for c in el:
            if _tag(c) == tag and c.text is not None and c.text.strip():
                return c.text.strip()
        return default

    def _block(self, el):
        return {"cycles": int(self._text(el, "cycles", "0")), "sizeheader": int(self._text(el, "sizeheader", "0")),
                "sizefooter": int(self._text(el, "sizefooter", "0")), "chunks": [self._chunk(c) for c in self._children(el, "chunk")]}

    def _chunk(self, el):
        streams = []
        for lump in self._children(el, "lump"):
            shift = _enum(self._text(lump, "shift", "undefined"), _SHIFT, "lump shift")
            for s in self._children(lump, "stream"):
                streams.append(self._stream(s, shift))
        return {"size_word": int(self._text(el, "sizeword", "1")), "count_words": int(self._text(el, "countwords", "1")),
                "big_endian": int(self._text(el, "endian", "little").lower() == "big"),
                "shift": _enum(self._text(el, "wordshift", "left"), _SHIFT, "word shift"),
                "padding": _enum(self._text(el, "padding", "none"), {"none": 0, "tail": 0, "head": 1}, "padding"),
                "n_streams": len(streams), "streams": streams}

    def _stream(self, el, lump_shift):
        rate, quant, bits = (int(self._text(el, t, d)) for t, d in (("ratefactor", "1"), ("quantization", "1"), ("packedbits", "1")))
        fmt = self._text(el, "format")
        if fmt is None:
            form, negate = (IQ if bits >= 2 * rate * quant else REAL), 0
        else:
            form, negate = parse_format(fmt)
        return {"name": el.get("id"), "packed_bits": bits, "rate_factor": rate, "quantization": quant,
                "encoding": self._text(el, "encoding", "TC").upper(), "format": form, "negate": negate,
                "alignment": _enum(self._text(el, "alignment", "undefined"), _ALIGN, "alignment"), "lump_shift": lump_shift}

    def find(self, stream_ids):
        """the first (file, block) whose block holds one of the streams, in the order of the reference's search (files, then the blocks of the file's
        lane: adapters/ion_gsms_signal_source.cc:125-186)"""
        for f in self.files:
            for block in self.lanes.get(f["lane"], []):
                if any(s["name"] in stream_ids for c in block["chunks"] for s in c["streams"]):
                    return f, block
        raise KeyError(f"no file of the metadata holds any of the streams {list(stream_ids)}")


class IonGsmsRecording:
    """A recording described by ION metadata: IonGsmsRecording(metadata_path, streams=[ids]) mirrors role.metadata_filename and role.streams
    (adapters/ion_gsms_signal_source.cc:63-64), finds the file, lane and block that hold the streams (:125-186) and hands out runs of whole cycles
    with every block's header and footer stripped, ready for IonLayout.push.  The file is `offset` bytes, then blocks of sizeheader + cycles cycles +
    sizefooter bytes; with cycles = 0 one block takes the rest of the file (gnuradio_blocks/ion_gsms.cc:76-87).
    Deviations from the reference, both on purpose: it adds the file offset twice when it seeks (ion_gsms.cc:45,56: block_offset is file.Offset()
    again), and it strips only the first block's header and no footer (:56, then reads on); here the data starts at offset + sizeheader and every
    block's header and footer are skipped.

    layout: the IonLayout of the block; streams: the indices of the requested streams in it, in the order asked; total_cycles; position (cycles)."""

    def __init__(self, metadata_path: str, streams):
        self.metadata = IonGsmsMetadata.parse(metadata_path)
        ids = [s.strip() for s in streams.split(",")] if isinstance(streams, str) else list(streams)
        f, block = self.metadata.find(ids)
        flat = [s for c in block["chunks"] for s in c["streams"]]
        self.layout = IonLayout(block["chunks"], flat)
        self.streams = [self.layout.index(i) for i in ids]
        self.path = os.path.join(os.path.dirname(os.path.abspath(metadata_path)), f["url"])
        self._offset, self._header, self._footer, self._cycles = f["offset"], block["sizeheader"], block["sizefooter"], block["cycles"]
        size = os.path.getsize(self.path)
        cb = self.layout.cycle_bytes
        if self._cycles == 0:
            self.total_cycles = max(0, size - self._offset - self._header - self._footer) // cb
            self._per_block = max(1, self.total_cycles)
        else:
            self._per_block = self._cycles
            self.total_cycles = max(0, size - self._offset) // (self._header + self._cycles * cb + self._footer) * self._cycles
        self.position = 0
        self._file = open(self.path, "rb")

    def close(self) -> None:
        self._file.close()
        self.layout.close()

    @property
    def remaining(self) -> int:
        return self.total_cycles - self.position

    def samples(self, stream) -> int:
        """samples of the stream in the whole recording"""
        return self.total_cycles * self.layout.stream_info(stream)[0]

    def read(self, n_cycles: int) -> np.ndarray:
        """the next min(n_cycles, remaining) whole cycles as bytes, headers and footers left out"""
        n = max(0, min(int(n_cycles), self.remaining))
        cb = self.layout.cycle_bytes
        out = np.empty(n * cb, np.uint8)
        done = 0
        while done < n:
            block, inside = divmod(self.position, self._per_block)
            take = min(n - done, self._per_block - inside)
            self._file.seek(self._offset + block * (self._header + self._per_block * cb + self._footer) + self._header + inside * cb)
            got = self._file.readinto(memoryview(out)[done * cb:(done + take) * cb])
            if got != take * cb:
                raise IOError(f"{self.path}: short read of {got} bytes for {take} cycles")
            done += take
            self.position += take
        return out

    def runs(self, n_cycles: int):
        """runs of up to n_cycles whole cycles, to the end of the recording"""
        while self.remaining:
            yield self.read(n_cycles)

    def push(self, rings, n_cycles: int, inverted_spectrum: bool = False) -> int:
        """the next run of whole cycles into the rings, requested stream i into rings[i]; returns the cycles pushed"""
        block = self.read(n_cycles)
        if block.size:
            self.layout.push(rings, self.streams, block, inverted_spectrum)
        return block.size // self.layout.cycle_bytes
