"""Host file handling of the reference's Labsat_Signal_Source (src/algorithms/signal_source/gnuradio_blocks/labsat23_source.cc, "ls.cc" below) for the
packed families that the device unpacks: which files make up a recording, where its samples start, and blocks of packed bytes for the ring pushes.
The samples themselves are never decoded here (but for the few in front of a round boundary after a seek): the bytes go to the device as they lie."""
from __future__ import annotations

import os

import numpy as np

from .sample_stream import PackedFormat, packed_decode_host, push_packed_multi


class LabSatRecording:
    """A LabSat recording on disk, by the file name the reference's `filename` property takes (generate_filename, ls.cc:333-361):
      x.ls4 / x.LS4    LabSat 4: the data file, with x.ini beside it (PackedFormat.from_ls4_ini)
      x.ls3w / x.LS3W  LabSat 3 Wideband: the data file, with x.ini beside it (PackedFormat.from_ls3w_ini)
      x.ls2 / x.LS2    LabSat 2: one file, a header (PackedFormat.from_labsat_header) and then 16-bit items
      anything else    LabSat 3: the base name of the sequence x_0000.LS3, x_0001.LS3, ...; the first file starts with the header, the following ones are
                       read from their first byte (ls.cc:1091-1103), and the data ends where the next file of the sequence is missing
    selected_channels: the reference's 1-based channel numbers; several only where the format is multi-band (LS3W, LS4), and for LS4 only channels of
    equal buffer size (ls.cc:898-906).  .format is the PackedFormat of the first one, .channels the 0-based list, .sample_rate the rate of the selected
    channels in samples per second (SMP of the .ini, divided by the channel's BW_DIV for LS4; None for LabSat 2 / 3, whose header does not carry it).

    seconds_to_skip (LS4 only, as in the reference: ls.cc:264-298) is turned into a position the way the reference does it for the selected channel:
    samples = int(seconds SMP / BW_DIV), bytes = samples 2 QUA / 8, whole buffers of BUF_SIZE first, then whole registers inside the buffer.  ROUNDING:
    the position is rounded down to a whole register, and at QUA 12 further down to a whole triple of registers (8 samples).  The reference can land
    inside a triple there (its data_index is any register), which puts every later sample at the wrong bit offset; this reader does not follow it.
    The round is taken from the selected channel alone; the reference sums per-channel buffer counts, which can differ by one between channels.

    The unit in which a recording is cut is the ROUND: a LabSat 4 round (one buffer per recorded channel), else one item or register.  No throttling."""

    def __init__(self, path: str, selected_channels=(1,), seconds_to_skip: float = 0.0, digital_io_enabled: bool = False):
        self.path = str(path)
        sel = [int(c) for c in selected_channels]
        if not sel or len(set(sel)) != len(sel):
            raise ValueError(f"selected_channels {selected_channels!r}: one or more distinct channel numbers")
        ext = os.path.splitext(self.path)[1]
        self.sample_rate = None
        self._skip_samples = 0
        if ext in (".ls4", ".LS4", ".ls3w", ".LS3W"):
            ini_path = os.path.splitext(self.path)[0] + ".ini"
            with open(ini_path) as f:
                text = f.read()
            self.files = [(self.path, 0, os.path.getsize(self.path))]
            if ext in (".ls4", ".LS4"):
                self.generation = "ls4"
                self.format = PackedFormat.from_ls4_ini(text, sel[0])
                cfg = PackedFormat.read_ls4_ini(text)
                for c in sel[1:]:
                    other = PackedFormat.from_ls4_ini(text, c)
                    if other.ls4_regs[c - 1] != self.format.ls4_regs[sel[0] - 1]:
                        raise ValueError(f"channels {sel[0]} and {c} hold {self.format.ls4_regs[sel[0] - 1]} and {other.ls4_regs[c - 1]} registers per round: "
                                         "selecting several channels of different bandwidth is not supported")
                div = cfg["bw_div"][sel[0] - 1]
                self.sample_rate = cfg["smp"] / div if cfg["smp"] else None
                self.round_bytes = self.format.ls4_round_bytes
                self.samples_per_round = self.format.ls4_samples_per_round()
                if seconds_to_skip > 0:
                    if not cfg["smp"]:
                        raise ValueError("seconds_to_skip needs the sample rate: the .ini has no SMP")
                    qua, buf = cfg["qua"], cfg["buf_size"][sel[0] - 1]
                    skip_bytes = int(seconds_to_skip * (cfg["smp"] / div)) * 2 * qua // 8
                    rounds, inside = divmod(skip_bytes, buf)
                    unit_bytes = 24 if qua == 12 else 8
                    self._skip_samples = rounds * self.samples_per_round + inside // unit_bytes * self.format.samples_per_item
            else:
                self.generation = "ls3w"
                self.format = PackedFormat.from_ls3w_ini(text, sel[0], digital_io_enabled)
                for c in sel[1:]:
                    PackedFormat.from_ls3w_ini(text, c, digital_io_enabled)
                import configparser
                ini = configparser.ConfigParser(strict=False, interpolation=None)
                ini.optionxform = str
                ini.read_string(text)
                smp = ini["config"].get("SMP")
                self.sample_rate = float(smp) if smp else None
                self.round_bytes, self.samples_per_round = 8, self.format.samples_per_item
        else:
            self.generation = "ls2" if ext in (".ls2", ".LS2") else "ls3"
            first = self.path if self.generation == "ls2" else f"{self.path}_0000.LS3"
            with open(first, "rb") as f:
                header = f.read(1024)
            self.format, offset = PackedFormat.from_labsat_header(header, sel[0])
            if len(sel) > 1:
                raise ValueError("a LabSat 2 / 3 file carries one RF channel")
            self.files = [(first, offset, os.path.getsize(first) - offset)]
            k = 1
            while self.generation == "ls3" and os.path.exists(f"{self.path}_{k:04d}.LS3"):
                name = f"{self.path}_{k:04d}.LS3"
                self.files.append((name, 0, os.path.getsize(name)))
                k += 1
            self.round_bytes, self.samples_per_round = 2, self.format.samples_per_item
        if seconds_to_skip > 0 and self.generation != "ls4":
            raise ValueError("seconds_to_skip applies to LabSat 4 recordings only, as in the reference")
        self.channels = [c - 1 for c in sel]
        # whole items per file (the reference drops a trailing partial item at every file's end: it reads whole int16 / registers)
        unit = self.round_bytes if self.generation != "ls4" else 1
        self.files = [(name, start, size // unit * unit) for name, start, size in self.files]
        total_bytes = sum(size for _, _, size in self.files)
        self.total_samples = total_bytes // self.round_bytes * self.samples_per_round   # (LS4: whole rounds)
        if self._skip_samples > self.total_samples:
            raise ValueError(f"the recording is shorter than the {seconds_to_skip} seconds to skip")
        self.position = self._skip_samples   # the next sample of the selected channels, counted from the recording's first

    @property
    def remaining(self) -> int:
        return self.total_samples - self.position

    def _bytes(self, offset: int, nbytes: int) -> np.ndarray:
        """nbytes of the recording's data bytes from `offset`, across the files of a sequence"""
        out = np.empty(nbytes, np.uint8)
        done = 0
        for name, start, size in self.files:
            if done == nbytes:
                break
            if offset >= size:
                offset -= size
                continue
            take = min(nbytes - done, size - offset)
            with open(name, "rb") as f:
                f.seek(start + offset)
                chunk = f.read(take)
            if len(chunk) != take:
                raise IOError(f"{name}: short read")
            out[done:done + take] = np.frombuffer(chunk, np.uint8)
            done += take
            offset = 0
        if done != nbytes:
            raise IOError("read past the end of the recording")
        return out

    def read_block(self, n_samples: int):
        """The packed bytes that hold the next min(n_samples, remaining) samples, and the index of the first of them inside that block: the block starts
        at a round boundary, so the index is non-zero only after a seek into a round (or a read that stopped inside one).  Advances the position.
        -> (uint8 array, first sample index); an empty array at the end of the data."""
        n = min(int(n_samples), self.remaining)
        if n <= 0:
            return np.empty(0, np.uint8), 0
        S = self.samples_per_round
        r0, r1 = self.position // S, (self.position + n + S - 1) // S
        first = self.position - r0 * S
        self.position += n
        return self._bytes(r0 * self.round_bytes, (r1 - r0) * self.round_bytes), first

    def push(self, rings, n_samples: int, inverted_spectrum: bool = False) -> int:
        """Append the next samples of selected channel i to rings[i] (one SampleStream per selected channel): at most n_samples, cut down to whole
        registers (whole triples for LS4 at QUA 12), fewer at the end of the data.  Several channels go through push_packed_multi, one pass over the
        block.  A packed block starts at a round boundary, so while the position stands inside a round (after seconds_to_skip, or after a push that ended
        inside one) the samples up to the round's end are decoded on the host and pushed as complex64: less than one round per call.
        -> the samples appended to every ring."""
        rings = list(rings)
        if len(rings) != len(self.channels):
            raise ValueError(f"{len(rings)} rings for {len(self.channels)} selected channels")
        S, unit = self.samples_per_round, self.format.samples_per_item
        n = min(int(n_samples), self.remaining) // unit * unit
        pushed = 0
        if n and self.position % S:
            head = min(n, S - self.position % S)
            data, first = self.read_block(head)
            for ring, ch in zip(rings, self.channels):
                x = packed_decode_host(self.format.with_channel(ch), data, first, head)
                ring.push(np.conj(x) if inverted_spectrum else x)
            pushed, n = head, n - head
        if n:
            data, first = self.read_block(n)
            assert first == 0
            if len(rings) == 1:
                rings[0].push_packed(self.format, data, inverted_spectrum, n_samples=n)
            else:
                push_packed_multi(rings, self.channels, self.format, data, inverted_spectrum, n_samples=n)
            pushed += n
        return pushed
