"""Telemetry on the device.  Galileo pages: the ctypes face of gsh_tlm_* (csrc/telemetry_viterbi.hip) and the frame synchroniser of
galileo_telemetry_decoder_gs restated on the host over device results.  GPS CNAV messages (L2C, L5): the ctypes face of gsh_cnav_*
(csrc/cnav_stream.hip), libswiftcnav's streaming decoder with its state kept on the device.

  symbols_from_records   the telemetry symbols of one channel's gsh_trk_epoch records
  TelemetryDecoder       one gsh_tlm handle: preamble scan and page-job tables on the device
  GalileoFrameSync       galileo_telemetry_decoder_gs.cc:953-1110: preamble search, lock, one page per period, loss of lock after 7 CRC failures
  CnavDecoder            one gsh_cnav handle: n channels of cnav_msg_decoder_add_symbol, as gps_l2c / gps_l5_telemetry_decoder_gs drive it

Not here: the contents of the pages and messages (ephemeris, TOW, HAS, OSNMA, Reed-Solomon, Gps_CNAV_Navigation_Message), a TelemetryDecoderInterface
adapter, GPS L1 C/A LNAV and SBAS (other decoders).
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _lib
from ._lib import (GSH_CNAV_QUANTISER_HARD, GSH_CNAV_QUANTISER_SOFT, CnavChannelState, CnavJob, CnavMessage)
from ._lib import (GSH_TLM_JOB_INAV_AUTO, GSH_TLM_JOB_INVERT, GSH_TLM_METRIC_FULL, GSH_TLM_METRIC_REFERENCE, TlmPageJob, TlmPageResult, check, fptr)

CRC_ERROR_LIMIT = 6  # galileo_telemetry_decoder_gs.cc:70
# frame type -> symbols after the preamble, information bits, preamble length, d_preamble_period_symbols, d_required_symbols, (crc_bits, crc_check)
FRAME = {
    1: dict(name="I/NAV", symbols=240, info_bits=114, preamble=10, period=250, required=510, crc=None),  # the page's first bit chooses
    2: dict(name="F/NAV", symbols=488, info_bits=238, preamble=12, period=500, required=512, crc=(214, 1)),  # galileo_fnav_message.cc:41-42
    3: dict(name="C/NAV", symbols=984, info_bits=486, preamble=16, period=1000, required=1016, crc=(462, 1)),  # galileo_cnav_message.cc:63-64
}
_METRIC = {"full": GSH_TLM_METRIC_FULL, "reference": GSH_TLM_METRIC_REFERENCE}


def symbols_from_records(records, component=0):
    """-> (symbols float32, sample_counters uint64) of one channel's gsh_trk_epoch records: p_data_accu[component] of every record whose symbol_flags
    bit 0 is set (a telemetry symbol was completed in that epoch), in order.  component 0 is Prompt_I (Galileo, GPS L2C), 1 is Prompt_Q, which the
    GPS L5 block reads (gps_l5_telemetry_decoder_gs.cc:213)"""
    keep = [r for r in records if r.symbol_flags & 1]
    return (np.array([r.p_data_accu[component] for r in keep], np.float32), np.array([r.sample_counter for r in keep], np.uint64))


def unpack_bits(words, info_bits: int):
    """the 16 MSB-first words of a gsh_tlm_page_result -> uint8 bits"""
    return np.unpackbits(np.asarray(words, np.uint32).astype(">u4").view(np.uint8))[:info_bits]


def job_table(jobs):
    """list of dicts (channel, frame_type, symbol_offset, flags, crc_bits, crc_check) -> gsh_tlm_page_job array"""
    table = (TlmPageJob * max(1, len(jobs)))()
    for t, j in zip(table, jobs):
        t.channel, t.frame_type, t.symbol_offset = int(j["channel"]), int(j["frame_type"]), int(j["symbol_offset"])
        t.flags, t.crc_bits, t.crc_check = int(j.get("flags", 0)), int(j.get("crc_bits", 0)), int(j.get("crc_check", 0))
    return table


class TelemetryDecoder:
    """gsh_tlm_*: n_channels Galileo page decoders on one device.  metric "full" (both symbols of a pair, every page from state 0) or "reference"
    (the reference's decoder as it runs: first symbol only, metrics carried from page to page of a channel)."""

    def __init__(self, n_channels: int, metric: str = "full", device: int = 0):
        self._lib = _lib.load()
        self._h = C.c_void_p()
        self.n_channels, self.metric = n_channels, metric
        check(self._lib.gsh_tlm_create(device, n_channels, _METRIC[metric], C.byref(self._h)))

    def close(self):
        if self._h:
            self._lib.gsh_tlm_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        self.close()

    def channel_reset(self, channel: int):
        check(self._lib.gsh_tlm_channel_reset(self._h, channel))

    def preamble_scan(self, frame_type: int, symbols):
        """int8 clipped correlation with the preamble at every position of the block (0 where the window leaves it)"""
        x = np.ascontiguousarray(symbols, np.float32)
        corr = np.zeros(len(x), np.int8)
        check(self._lib.gsh_tlm_preamble_scan(self._h, frame_type, fptr(x), len(x), corr.ctypes.data_as(C.POINTER(C.c_int8))))
        return corr

    def _results(self, jobs, res):
        out = []
        for j, r in zip(jobs, res):
            words = np.array(r.bits[:], np.uint32)
            out.append(dict(bits=unpack_bits(words, FRAME[int(j["frame_type"])]["info_bits"]), words=words, crc_register=int(r.crc_register), crc_ok=int(r.crc_ok)))
        return out

    def decode_pages(self, symbols, jobs):
        """symbols: host float32; jobs: list of dicts -> list of dicts (bits, words, crc_register, crc_ok), one per job"""
        x = np.ascontiguousarray(symbols, np.float32)
        res = (TlmPageResult * max(1, len(jobs)))()
        check(self._lib.gsh_tlm_decode_pages(self._h, fptr(x), len(x), job_table(jobs), len(jobs), res))
        return self._results(jobs, res)

    def decode_pages_device(self, device_ptr: int, n_symbols: int, jobs):
        """the same over n_symbols float32 resident on the decoder's device (e.g. a torch tensor's data_ptr())"""
        res = (TlmPageResult * max(1, len(jobs)))()
        check(self._lib.gsh_tlm_decode_pages_device(self._h, C.c_void_p(device_ptr), n_symbols, job_table(jobs), len(jobs), res))
        return self._results(jobs, res)

    def time_decode_pages(self, symbols, jobs, reps: int = 20) -> float:
        """HIP-event average milliseconds per launch of the table"""
        x = np.ascontiguousarray(symbols, np.float32)
        ms = C.c_float()
        check(self._lib.gsh_tlm_time_decode_pages(self._h, fptr(x), len(x), job_table(jobs), len(jobs), reps, C.byref(ms)))
        return float(ms.value)


@dataclass
class Page:
    channel: int
    preamble_index: int  # symbol index, counted from the channel's first pushed symbol, of the preamble in front of the page
    inverted: bool       # d_flag_PLL_180_deg_phase_locked
    bits: np.ndarray     # uint8, the information bits
    crc_ok: bool         # the block's crc_ok; for I/NAV the latch of Galileo_Inav_Message::split_page
    crc_register: int


class _Channel:
    def __init__(self):
        self.buf = np.zeros(0, np.float32)
        self.base = 0        # symbol index of buf[0]
        self.stat = 0        # d_stat
        self.pidx = 0        # position of the last preamble stamp (d_preamble_index, counted in window positions)
        self.next_p = 0      # next window position the state machine looks at in states 0 and 1
        self.err = 0         # d_CRC_error_counter
        self.inverted = False
        self.even_arrived = 0  # d_flag_even_word_arrived
        self.latch = False     # Galileo_Inav_Message::flag_CRC_test


class GalileoFrameSync:
    """The frame synchroniser of galileo_telemetry_decoder_gs (:953-1110) for n_channels channels of one frame type.  The block looks, once per symbol,
    at a window of d_required_symbols + 1 symbols whose OLDEST preamble-length symbols it correlates; here window position p is the symbol index of that
    oldest symbol, and a push walks all the positions its symbols complete:
      state 0  |corr[p]| = preamble length -> stamp p, state 1
      state 1  a second hit exactly one period after the stamp -> state 2, the sign of that correlation is the 180 deg flag; a hit further away -> state 0
      state 2  one page every period (no correlation), decoded from the symbols after the preamble position; more than CRC_ERROR_LIMIT failures in a
               row -> state 0
    The I/NAV verdict is the latch of Galileo_Inav_Message::split_page: it changes only when an odd part follows an even part.
    Each push scans on the device and submits the pages the state implies as one job table, then walks the results; where the error counter passes the
    limit the pages after that point are dropped and scanning resumes there.  Where a dropped page would have moved state the device keeps per channel
    (the carried metrics of the "reference" metric, the I/NAV CRC chain), a table holds no more pages of a channel than can pass before the limit."""

    def __init__(self, frame_type: int, n_channels: int, metric: str = "full", device: int = 0, engine=None):
        if frame_type not in FRAME:
            raise ValueError(f"unknown frame type {frame_type}")
        self.frame_type, self.n_channels, self.metric = frame_type, n_channels, metric
        self.f = FRAME[frame_type]
        self.engine = engine if engine is not None else TelemetryDecoder(n_channels, metric, device)
        self.ch = [_Channel() for _ in range(n_channels)]

    def close(self):
        self.engine.close()

    def state(self, channel: int) -> int:
        return self.ch[channel].stat

    def _search(self, c: _Channel, corr, p_first: int, p_max: int):
        """states 0 and 1 over the hits among positions c.next_p..p_max; corr[0] is position p_first"""
        f = self.f
        lo = c.next_p - p_first
        hits = np.nonzero(np.abs(corr[lo:p_max - p_first + 1].astype(np.int32)) >= f["preamble"])[0] + lo + p_first
        for p in hits:
            p = int(p)
            if c.stat == 0:
                c.pidx, c.stat = p, 1
            else:
                diff = p - c.pidx
                if diff == f["period"]:
                    c.pidx, c.err, c.stat = p, 0, 2
                    c.inverted = bool(corr[p - p_first] < 0)
                    c.next_p = p + 1
                    return
                if diff > f["period"]:
                    c.stat = 0
        c.next_p = p_max + 1

    def push(self, blocks):
        """blocks: {channel: float32 symbols, appended to the channel's stream} -> list of Page, per channel in stream order"""
        f = self.f
        pages = []
        active = []
        for chn, sym in blocks.items():
            c = self.ch[chn]
            c.buf = np.concatenate([c.buf, np.asarray(sym, np.float32)])
            active.append(chn)
        corr = {}
        while True:
            jobs, owners = [], []
            offset, parts = 0, []
            for chn in active:
                c = self.ch[chn]
                p_max = c.base + len(c.buf) - f["required"] - 1  # the newest complete window
                if c.stat != 2 and c.next_p <= p_max:
                    if chn not in corr:
                        corr[chn] = (c.base, self.engine.preamble_scan(self.frame_type, c.buf))
                    self._search(c, corr[chn][1], corr[chn][0], p_max)
                if c.stat != 2:
                    continue
                n_pages = (p_max - c.pidx) // f["period"] if p_max >= c.pidx else 0
                if self.frame_type == 1 or self.metric == "reference":
                    n_pages = min(n_pages, CRC_ERROR_LIMIT + 1 - c.err)
                if n_pages <= 0:
                    continue
                parts.append(c.buf)
                for k in range(1, n_pages + 1):
                    q = c.pidx + k * f["period"]
                    job = dict(channel=chn, frame_type=self.frame_type, symbol_offset=offset + q - c.base + f["preamble"],
                               flags=GSH_TLM_JOB_INVERT if c.inverted else 0)
                    if self.frame_type == 1:
                        job["flags"] |= GSH_TLM_JOB_INAV_AUTO
                    else:
                        job["crc_bits"], job["crc_check"] = f["crc"]
                    jobs.append(job)
                    owners.append((chn, q))
                offset += len(c.buf)
            if not jobs:
                break
            results = self.engine.decode_pages(np.concatenate(parts), jobs)
            lost = set()
            for (chn, q), r in zip(owners, results):
                if chn in lost:
                    continue  # dropped: the block would have been searching again
                c = self.ch[chn]
                if self.frame_type == 1:
                    if r["bits"][0] == 1:
                        if c.even_arrived == 1:
                            c.latch = r["crc_ok"] == 1
                        c.even_arrived = 0
                    else:
                        c.even_arrived = 1
                    ok = c.latch
                else:
                    ok = r["crc_ok"] == 1
                c.pidx = q
                pages.append(Page(chn, q, c.inverted, r["bits"], bool(ok), r["crc_register"]))
                if ok:
                    c.err = 0
                else:
                    c.err += 1
                    if c.err > CRC_ERROR_LIMIT:
                        c.stat, c.next_p = 0, q + 1
                        lost.add(chn)
        for chn in active:
            c = self.ch[chn]
            keep = c.next_p if c.stat != 2 else c.pidx + f["period"]  # the oldest symbol a later push can still look at
            drop = min(max(keep - c.base, 0), len(c.buf))
            c.buf, c.base = c.buf[drop:], c.base + drop
        return pages


@dataclass
class CnavMessageOut:
    channel: int
    symbol_index: int  # counted from the channel's first pushed symbol: the symbol that completed the message
    bits: np.ndarray   # uint8, the 300 bits, un-inverted
    words: np.ndarray  # uint32, the same MSB first in 10 words
    delay: int         # cnav_msg.c:344, in symbols
    prn: int
    msg_id: int
    tow: int           # in 6 s units
    alert: bool
    part: int          # 1 or 2: which of the two decoders delivered
    invert: bool       # that part's invert flag
    phase_locked_180: bool  # part1.invert | part2.invert: d_flag_PLL_180_deg_phase_locked of both blocks (gps_l5_telemetry_decoder_gs.cc:227-234)
    time_of_symbol: float   # the block's time of the current symbol: seconds for L2C, milliseconds for L5


def cnav_result_capacity(n_symbols: int) -> int:
    """GSH_CNAV_RESULT_CAPACITY: the messages n symbols can deliver (576 symbols apart at the closest)"""
    return 1 if n_symbols == 0 else (n_symbols + 575) // 576


def cnav_job_table(jobs):
    """list of dicts (channel, symbol_offset, n_symbols, result_offset, result_capacity) -> gsh_cnav_job array"""
    table = (CnavJob * max(1, len(jobs)))()
    for t, j in zip(table, jobs):
        t.channel, t.symbol_offset, t.n_symbols = int(j["channel"]), int(j["symbol_offset"]), int(j["n_symbols"])
        t.result_offset, t.result_capacity = int(j["result_offset"]), int(j["result_capacity"])
    return table


class CnavDecoder:
    """gsh_cnav_*: n_channels GPS CNAV message decoders on one device, each the pair of sliding-window Viterbi decoders and message-lock machines of
    libswiftcnav's cnav_msg_decoder_t, kept on the device from push to push.  signal "L2C" or "L5" only chooses the block's time formula; quantiser
    "hard" is what both blocks do ((x > 0) * 255), ("soft", scale) maps [-scale, scale] onto 0..255."""

    def __init__(self, n_channels: int, signal: str = "L2C", quantiser="hard", device: int = 0):
        self._lib = _lib.load()
        self._h = C.c_void_p()
        if signal not in ("L2C", "L5"):
            raise ValueError(f"unknown signal {signal!r}")
        if quantiser == "hard":
            mode, scale = GSH_CNAV_QUANTISER_HARD, 1.0
        elif isinstance(quantiser, tuple) and len(quantiser) == 2 and quantiser[0] == "soft":
            mode, scale = GSH_CNAV_QUANTISER_SOFT, float(quantiser[1])
        else:
            raise ValueError(f"unknown quantiser {quantiser!r}")
        self.n_channels, self.signal, self.quantiser = n_channels, signal, quantiser
        self.pushed = [0] * n_channels  # symbols each channel has taken since its reset
        check(self._lib.gsh_cnav_create(device, n_channels, mode, scale, C.byref(self._h)))

    def close(self):
        if self._h:
            self._lib.gsh_cnav_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        self.close()

    def channel_reset(self, channel: int):
        check(self._lib.gsh_cnav_channel_reset(self._h, channel))
        self.pushed[channel] = 0

    def get_state(self, channel: int) -> CnavChannelState:
        state = CnavChannelState()
        check(self._lib.gsh_cnav_channel_get_state(self._h, channel, C.byref(state)))
        return state

    def set_state(self, channel: int, state: CnavChannelState, pushed: int = 0):
        """puts a whole decoder state into a channel; `pushed` is the symbol count the channel's later indices continue from"""
        check(self._lib.gsh_cnav_channel_set_state(self._h, channel, C.byref(state)))
        self.pushed[channel] = pushed

    def time_of_symbol(self, tow: int, delay: int) -> float:
        if self.signal == "L2C":
            return tow * 6 + delay * 0.02 + 12 * 0.02  # gps_l2c_telemetry_decoder_gs.cc:287, seconds
        return float(tow * 6000 + (delay + 12) * 10)   # gps_l5_telemetry_decoder_gs.cc:308, milliseconds

    def _layout(self, blocks, dtype):
        chans = list(blocks)
        arrays = [np.ascontiguousarray(blocks[c], dtype).reshape(-1) for c in chans]
        jobs, at, res = [], 0, 0
        for c, a in zip(chans, arrays):
            cap = cnav_result_capacity(len(a))
            jobs.append(dict(channel=c, symbol_offset=at, n_symbols=len(a), result_offset=res, result_capacity=cap))
            at, res = at + len(a), res + cap
        return jobs, (np.concatenate(arrays) if arrays else np.zeros(0, dtype)), res

    def _collect(self, jobs, table, counts):
        out = []
        for j, n in zip(jobs, counts):
            c = j["channel"]
            for r in table[j["result_offset"]:j["result_offset"] + n]:
                words = np.array(r.bits[:], np.uint32)
                out.append(CnavMessageOut(c, self.pushed[c] + int(r.symbol_index), np.unpackbits(words.astype(">u4").view(np.uint8))[:300], words,
                                          int(r.delay), int(r.prn), int(r.msg_id), int(r.tow), bool(r.alert), int(r.part), bool(r.invert),
                                          bool(r.invert_or), self.time_of_symbol(int(r.tow), int(r.delay))))
            self.pushed[c] += j["n_symbols"]
        return out

    def push_jobs(self, entry, symbols_arg, n_symbols, jobs, n_results):
        """one launch over a job table (list of dicts, see cnav_job_table) -> list of CnavMessageOut, per job in table order.  GshError
        (GSH_ERR_STATE) if a channel delivered more than its job's capacity, which only an imported state can cause"""
        table = (CnavMessage * max(1, n_results))()
        counts = (C.c_int32 * max(1, len(jobs)))()
        check(entry(self._h, symbols_arg, n_symbols, cnav_job_table(jobs), len(jobs), table, n_results, counts))
        return self._collect(jobs, table, list(counts)[:len(jobs)])

    def push(self, blocks):
        """blocks: {channel: float symbols, appended to the channel's stream}, through the quantiser -> list of CnavMessageOut"""
        jobs, x, n_results = self._layout(blocks, np.float32)
        return self.push_jobs(self._lib.gsh_cnav_push_f32, fptr(x), len(x), jobs, n_results)

    def push_u8(self, blocks):
        """the same over symbols as the library takes them: uint8, 0x00 a certain 0, 0xFF a certain 1"""
        jobs, x, n_results = self._layout(blocks, np.uint8)
        return self.push_jobs(self._lib.gsh_cnav_push_u8, x.ctypes.data_as(C.POINTER(C.c_uint8)), len(x), jobs, n_results)

    def push_device(self, device_ptr: int, n_symbols: int, spans):
        """spans: {channel: (offset, count)} into n_symbols float32 resident on the decoder's device (e.g. a torch tensor's data_ptr())"""
        jobs, res = [], 0
        for c, (offset, count) in spans.items():
            cap = cnav_result_capacity(count)
            jobs.append(dict(channel=c, symbol_offset=offset, n_symbols=count, result_offset=res, result_capacity=cap))
            res += cap
        return self.push_jobs(self._lib.gsh_cnav_push_f32_device, C.c_void_p(device_ptr), n_symbols, jobs, res)

    def time_push(self, blocks, reps: int = 10) -> float:
        """HIP-event average milliseconds per launch of uint8 blocks; the channels' states are as before afterwards"""
        jobs, x, _ = self._layout(blocks, np.uint8)
        ms = C.c_float()
        check(self._lib.gsh_cnav_time_push(self._h, x.ctypes.data_as(C.POINTER(C.c_uint8)), len(x), cnav_job_table(jobs), len(jobs), reps, C.byref(ms)))
        return float(ms.value)
