"""GPS CNAV messages on the device (csrc/cnav_stream.hip through gnss_sdr_amd.telemetry.CnavDecoder) against libswiftcnav itself
(tests/golden/cnav.npz) and against the host build of the same header (tests/cnav_host.py): deliveries and decoder states, bit for bit."""
import ctypes as C

import numpy as np
import pytest

import kernel_metadata
from cnav_host import (ALIGNED, ALIGNED_WINDOWS, pending_delivery_state, messages_array, MESSAGE, PIECES, HostCnavChannel, cuts, golden, host_quantise, raise_metrics, state_bytes, state_from_bytes)
from gnss_sdr_amd import _lib
from gnss_sdr_amd.telemetry import CnavDecoder, cnav_job_table, cnav_result_capacity

pytestmark = pytest.mark.gpu
CASES, RAISE_AT, RAISE_BY = golden()
PLAIN = [n for n in CASES if n != "normalise"]


def records(messages, channel):
    """the CnavMessageOut of one channel -> MESSAGE records, symbol_index counted from the channel's first symbol"""
    mine = [m for m in messages if m.channel == channel]
    out = np.zeros(len(mine), MESSAGE)
    for r, m in zip(out, mine):
        r["bits"], r["symbol_index"], r["delay"], r["tow"] = m.words, m.symbol_index, m.delay, m.tow
        r["prn"], r["msg_id"], r["alert"], r["part"], r["invert"], r["invert_or"] = m.prn, m.msg_id, m.alert, m.part, m.invert, m.phase_locked_180
        assert np.array_equal(np.packbits(np.concatenate([m.bits, np.zeros(20, np.uint8)])).view(">u4"), m.words)
    return out


def same_messages(got, want, where):
    assert len(got) == len(want), (where, len(got), len(want))
    for f in want.dtype.names:
        assert np.array_equal(got[f], want[f]), (where, f)


def same_as_golden(dec, channel, messages, name):
    same_messages(records(messages, channel), CASES[name][1], name)
    assert np.array_equal(state_bytes(dec.get_state(channel)), CASES[name][2]), name


def test_every_golden_case_one_channel_each_in_one_launch(gpu):
    dec = CnavDecoder(len(PLAIN), "L2C", "hard", gpu)
    msgs = dec.push_u8({c: CASES[name][0] for c, name in enumerate(PLAIN)})
    for c, name in enumerate(PLAIN):
        same_as_golden(dec, c, msgs, name)
    first = [m for m in msgs if m.channel == 0][0]
    assert first.time_of_symbol == first.tow * 6 + first.delay * 0.02 + 12 * 0.02 and first.symbol_index == 703
    l5 = CnavDecoder(1, "L5", "hard", gpu)
    m5 = l5.push_u8({0: CASES[PLAIN[0]][0]})[0]
    assert m5.time_of_symbol == m5.tow * 6000 + (m5.delay + 12) * 10 and np.array_equal(m5.words, first.words)
    dec.close()
    l5.close()


def test_ragged_pushes_equal_one_push(gpu):
    """one channel per piece size and one with random pieces, two streams (part 1 and part 2 hold the lock), each whole stream in pieces of that
    size: the channels of piece size 1 go symbol by symbol through all their 3 601 and 3 524 symbols, one launch per symbol"""
    rng = np.random.default_rng(11)
    plans = []  # (case, cuts)
    for name in ("hard_p1_inv_s05", "false_preamble_first"):
        n = len(CASES[name][0])
        for piece in PIECES:
            plans.append((name, cuts(n, piece)))
        plans.append((name, cuts(n, rng=rng)))
    dec = CnavDecoder(len(plans), "L2C", "hard", gpu)
    msgs = []
    for r in range(max(len(p[1]) for p in plans)):
        msgs += dec.push_u8({c: CASES[name][0][pieces[r][0]:pieces[r][1]] for c, (name, pieces) in enumerate(plans) if r < len(pieces)})
    for c, (name, _) in enumerate(plans):
        same_as_golden(dec, c, msgs, name)
    dec.close()


def test_a_single_symbol_completes_a_decode_block(gpu):
    sym = CASES["hard_p0_up_s00"][0]
    dec, host = CnavDecoder(1, "L2C", "hard", gpu), HostCnavChannel()
    assert dec.push_u8({0: sym[:127]}) == [] and len(host.push(sym[:127])) == 0
    before = dec.get_state(0)
    assert (before.part[0].n_symbols, before.part[0].n_decoded, before.part[0].decisions_index, before.part[0].flags & 16) == (127, 0, 0, 16)
    assert np.array_equal(state_bytes(before), state_bytes(host.state))
    dec.push_u8({0: sym[127:128]})   # part 1's block of 128; part 2, primed with one symbol, had its own one symbol earlier
    host.push(sym[127:128])
    after = dec.get_state(0)
    assert (after.part[0].n_symbols, after.part[0].flags & 16) == (0, 0) and after.part[0].n_decoded > 0 and any(after.part[0].decisions)
    assert (before.part[1].n_symbols, before.part[1].flags & 16) == (0, 0)
    assert np.array_equal(state_bytes(after), state_bytes(host.state))
    dec.close()


def test_pushes_that_begin_on_a_delivery_symbol_lose_nothing(gpu):
    """messages complete 576 and 640 symbols apart in turn, so a push of 577 symbols can hold two and one of 1 793 four: more than n / 600 + 1.
    One channel per window, three launches: up to the window, the window, the rest"""
    sym, want, _ = CASES[ALIGNED]
    dec = CnavDecoder(len(ALIGNED_WINDOWS), "L2C", "hard", gpu)
    msgs = dec.push_u8({c: sym[:start] for c, (start, _, _) in enumerate(ALIGNED_WINDOWS)})
    inside = dec.push_u8({c: sym[start:start + length] for c, (start, length, _) in enumerate(ALIGNED_WINDOWS)})
    for c, (start, length, n) in enumerate(ALIGNED_WINDOWS):
        assert len(records(inside, c)) == n, (start, length)
    msgs += inside + dec.push_u8({c: sym[start + length:] for c, (start, length, _) in enumerate(ALIGNED_WINDOWS)})
    for c in range(len(ALIGNED_WINDOWS)):
        same_as_golden(dec, c, msgs, ALIGNED)
    dec.close()


def test_an_imported_state_that_delivers_past_the_capacity_is_reported(gpu, gsh):
    """only a state put in by set_state with a message's worth of decoded bits can deliver faster than the capacity rule: the first messages are
    written, the count says how many there were, the call returns GSH_ERR_STATE and the channel has moved on exactly as the host's"""
    sym, want, _ = CASES[ALIGNED]
    state, pushed = pending_delivery_state(CASES)
    dec = CnavDecoder(2, "L2C", "hard", gpu)
    dec.set_state(1, state, pushed=pushed)
    span = np.ascontiguousarray(sym[pushed:pushed + 320])
    jobs = [dict(channel=1, symbol_offset=0, n_symbols=320, result_offset=1, result_capacity=1)]
    table, counts = (_lib.CnavMessage * 3)(), (C.c_int32 * 1)()
    rc = gsh.gsh_cnav_push_u8(dec._h, span.ctypes.data_as(C.POINTER(C.c_uint8)), 320, cnav_job_table(jobs), 1, table, 3, counts)
    assert rc == 4 and b"delivered 2 messages" in gsh.gsh_last_error() and counts[0] == 2   # GSH_ERR_STATE
    got = messages_array(table, 3)
    assert got["symbol_index"].tolist() == [0, 0, 0] and got["tow"].tolist() == [0, 1001, 0]   # one written, in its place; nothing beside it
    assert np.array_equal(got["bits"][1], want["bits"][1])
    host = HostCnavChannel(state)
    host.push(span, capacity=1)
    assert host.delivered == 2 and np.array_equal(state_bytes(dec.get_state(1)), state_bytes(host.state))
    dec.set_state(1, state, pushed=pushed)
    with pytest.raises(_lib.GshError):
        dec.push_u8({1: span})   # the Python face lays out (320 + 575) / 576 = 1 entry, and raises
    dec.set_state(1, state, pushed=pushed)
    table, counts = (_lib.CnavMessage * 3)(), (C.c_int32 * 1)()
    jobs[0]["result_capacity"] = 2   # room for both: no error
    assert gsh.gsh_cnav_push_u8(dec._h, span.ctypes.data_as(C.POINTER(C.c_uint8)), 320, cnav_job_table(jobs), 1, table, 3, counts) == 0
    assert counts[0] == 2 and messages_array(table, 3)["symbol_index"].tolist() == [0, 0, 319]
    dec.close()


def test_67_channels_at_scattered_places_in_shuffled_order_and_a_second_launch(gpu):
    rng = np.random.default_rng(67)
    names = [PLAIN[i] for i in rng.permutation(len(PLAIN))[:67]]
    split = {c: int(rng.integers(1, len(CASES[n][0]))) for c, n in enumerate(names)}
    dec = CnavDecoder(67, "L2C", "hard", gpu)
    u8 = C.POINTER(C.c_uint8)
    msgs = []
    for launch in range(2):
        order = rng.permutation(67)
        gaps = rng.integers(0, 50, 68)
        parts, jobs, at, res = [], [], 0, 0
        for k, c in enumerate(order):   # the shared array: gap, channel's span, gap, ...
            c = int(c)
            sym = CASES[names[c]][0]
            span = sym[:split[c]] if launch == 0 else sym[split[c]:]
            parts += [np.full(gaps[k], 0x5A, np.uint8), span]
            at += int(gaps[k])
            cap = cnav_result_capacity(len(span))
            jobs.append(dict(channel=c, symbol_offset=at, n_symbols=len(span), result_offset=res, result_capacity=cap))
            at, res = at + len(span), res + cap + int(k % 3)   # unused result entries between the slices
        array = np.concatenate(parts + [np.full(gaps[67], 0x5A, np.uint8)])
        jobs = [jobs[i] for i in rng.permutation(67)]
        msgs += dec.push_jobs(dec._lib.gsh_cnav_push_u8, array.ctypes.data_as(u8), len(array), jobs, res + 4)
    for c, name in enumerate(names):
        same_as_golden(dec, c, msgs, name)
    dec.close()


@pytest.mark.parametrize("quantiser", ["hard", ("soft", 1.0), ("soft", 0.37)])
def test_float_symbols_through_the_quantiser(gpu, quantiser):
    import torch
    names = ["soft_p0_up_s05", "soft_p1_inv_s07", "soft_p2_up_s10"]
    rng = np.random.default_rng(3)
    scale = 1.0 if quantiser == "hard" else quantiser[1]
    floats = {c: ((CASES[n][0].astype(np.float32) - np.float32(127.5)) / np.float32(120.0) + rng.normal(0, 0.05, len(CASES[n][0])).astype(np.float32)) *
              np.float32(scale) for c, n in enumerate(names)}
    bytes_ = {c: host_quantise(x, 0 if quantiser == "hard" else 1, scale) for c, x in floats.items()}
    assert all(len(np.unique(b)) == 2 if quantiser == "hard" else len(np.unique(b)) > 200 for b in bytes_.values())
    a, b, d = (CnavDecoder(3, "L5", q, gpu) for q in (quantiser, "hard", quantiser))
    got, want = a.push(floats), b.push_u8(bytes_)
    whole = np.concatenate([floats[c] for c in range(3)])
    t = torch.from_numpy(whole).to(f"cuda:{gpu}")
    torch.cuda.synchronize()
    spans, at = {}, 0
    for c in range(3):
        spans[c] = (at, len(floats[c]))
        at += len(floats[c])
    resident = d.push_device(t.data_ptr(), len(whole), spans)
    assert sum(len(records(want, c)) for c in range(3)) >= 5
    for c in range(3):
        same_messages(records(got, c), records(want, c), (quantiser, c))
        same_messages(records(resident, c), records(want, c), (quantiser, c, "device"))
        assert np.array_equal(state_bytes(a.get_state(c)), state_bytes(b.get_state(c)))
        assert np.array_equal(state_bytes(d.get_state(c)), state_bytes(b.get_state(c)))
    for x in (a, b, d):
        x.close()


def test_a_state_moves_between_device_and_host_in_mid_stream(gpu):
    name, at = "loss_p1", 5003   # part 2 holds the lock at the cut, part 1 is starved
    sym, want, want_state = CASES[name]
    dec = CnavDecoder(2, "L2C", "hard", gpu)
    first = dec.push_u8({1: sym[:at]})
    state = dec.get_state(1)
    assert state.part[1].flags & 4 and not state.part[0].flags & 4
    host = HostCnavChannel(state)
    host.pushed = at
    same_messages(np.concatenate([records(first, 1), host.push(sym[at:])]), want, "device to host")
    assert np.array_equal(state_bytes(host.state), want_state)
    # and back: the host's first half into channel 0 of the device
    host = HostCnavChannel()
    head = host.push(sym[:at])
    dec.set_state(0, host.state, pushed=at)
    same_messages(np.concatenate([head, records(dec.push_u8({0: sym[at:]}), 0)]), want, "host to device")
    assert np.array_equal(state_bytes(dec.get_state(0)), want_state)
    bad = state_from_bytes(state_bytes(host.state))
    bad.part[0].decisions_index = 64
    with pytest.raises(_lib.GshError):
        dec.set_state(0, bad)
    assert np.array_equal(state_bytes(dec.get_state(0)), want_state)
    dec.close()


def test_normalisation_on_the_device_through_set_state(gpu):
    sym = CASES["normalise"][0]
    dec = CnavDecoder(1, "L2C", "hard", gpu)
    first = dec.push_u8({0: sym[:RAISE_AT]})
    state = dec.get_state(0)
    raise_metrics(state, RAISE_BY)
    dec.set_state(0, state, pushed=RAISE_AT)
    assert max(dec.get_state(0).part[1].old_metrics) > 1 << 30
    msgs = first + dec.push_u8({0: sym[RAISE_AT:]})
    same_as_golden(dec, 0, msgs, "normalise")
    assert max(dec.get_state(0).part[0].old_metrics) < 1 << 29 and max(dec.get_state(0).part[1].old_metrics) < 1 << 29
    dec.close()


def test_range_errors_of_a_live_handle_launch_nothing(gpu, gsh):
    name = "hard_p3_inv_s00"
    sym = CASES[name][0]
    dec = CnavDecoder(2, "L2C", "hard", gpu)
    head = dec.push_u8({0: sym[:1000]})
    before = state_bytes(dec.get_state(0))
    u8 = C.POINTER(C.c_uint8)
    rest = np.ascontiguousarray(sym[1000:])
    good = dict(channel=0, symbol_offset=0, n_symbols=len(rest), result_offset=0, result_capacity=cnav_result_capacity(len(rest)))
    for why, jobs in (("capacity", [dict(good, result_capacity=len(rest) // 600 + 1 - 1)]),
                      ("capacity of n / 600 + 1", [dict(good, symbol_offset=3, n_symbols=577, result_capacity=1)]),
                      ("duplicate channel", [good, dict(good, result_offset=8)]),
                      ("channel", [dict(good, channel=2)])):
        with pytest.raises(_lib.GshError):
            dec.push_jobs(gsh.gsh_cnav_push_u8, rest.ctypes.data_as(u8), len(rest), jobs, 16)
        assert np.array_equal(state_bytes(dec.get_state(0)), before), why
    msgs = head + dec.push_u8({0: rest})
    assert len(head) == 1
    same_as_golden(dec, 0, msgs, name)
    with pytest.raises(_lib.GshError):
        dec.channel_reset(2)
    dec.channel_reset(0)
    assert np.array_equal(state_bytes(dec.get_state(0)), state_bytes(HostCnavChannel().state))
    dec.close()


def test_timing_entry_leaves_the_channels_as_they_were(gpu):
    sym = CASES["hard_p0_up_s00"][0]
    dec = CnavDecoder(3, "L2C", "hard", gpu)
    dec.push_u8({c: sym[:500 + c] for c in range(3)})
    before = [state_bytes(dec.get_state(c)) for c in range(3)]
    assert dec.time_push({c: sym[500 + c:] for c in range(3)}, reps=2) > 0.0
    assert all(np.array_equal(state_bytes(dec.get_state(c)), before[c]) for c in range(3))
    dec.close()


def test_the_kernels_use_no_scratch():
    mine = {n: k for n, k in kernel_metadata.kernels(_lib.LIB_PATH).items() if "cnav_stream_kernel" in n}
    assert len(mine) == 2, list(mine)   # uint8 and float input
    for n, k in mine.items():
        assert k[".private_segment_fixed_size"] == 0 and k[".vgpr_count"] <= 128 and k[".group_segment_fixed_size"] <= 4096, (n, k)
