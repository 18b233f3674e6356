"""CPU tests of the signal generator's model and table builders against tests/golden/siggen.npz, the output of the reference's own
signal_generator_c block (minted by tests/golden/make_golden_siggen.py; data_flag and noise_flag false):

  * the numpy float64 model (tests/siggen_reference.py) reproduces the block's outputs within ref_vs_model_max + 1e-6 sum |amplitudes| --
    ref_vs_model_max is the reference's own float32 phase accumulation, recorded in the fixture;
  * the Python table builders (gnss_sdr_amd.signal_generator) reproduce the fixture's tables, delays and sign sequences EXACTLY: they are
    sampled +-1 chips times one float32 scale, any difference is a bug in the restatement."""
import os

import numpy as np
import pytest

import siggen_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "siggen.npz")))


def fixture_tables(g, tag):
    iq = g[f"{tag}_tables_iq"].astype(np.float32)
    return (iq[..., 0] + 1j * iq[..., 1]).astype(np.complex64)


def built_satellites(g, tag, scaled=False):
    """the case's satellites from the Python builders (the block's noise_flag false: unscaled)"""
    from gnss_sdr_amd import signal_generator as SG
    sats = []
    for s, prn in enumerate(g[f"{tag}_prn"]):
        kw = dict(fs=int(g[f"{tag}_fs"]), delay_chips=int(g[f"{tag}_delay_chips"][s]), doppler_hz=float(g[f"{tag}_doppler_hz"][s]),
                  cn0_db=float(g[f"{tag}_cn0_db"][s]) if scaled else None)
        if tag == "gps":
            sats.append(SG.gps_l1_ca_satellite(int(prn), **kw))
        else:
            prim = g["e5a_primary_iq"][s].astype(np.float32)
            sats.append(SG.galileo_e5a_satellite(prim[:, 0] + 1j * prim[:, 1], g["e5a_secondary_i"], g["e5a_secondary_q"][s],
                                                 delay_sec=int(g["e5a_delay_sec"][s]), **kw))
    return sats


def test_fixture_holds_what_the_issue_asks(golden):
    g = golden
    assert g["gps_out"].dtype == np.complex64 and g["gps_out"].size == 3 * 4000 and int(g["gps_fs"]) == 4000000
    assert list(g["gps_prn"]) == [1, 10, 25] and list(g["gps_delay_chips"]) == [0, 600, 1022] and list(g["gps_doppler_hz"]) == [-3250.0, 750.0, 4999.0]
    assert len(set(g["gps_cn0_db"].tolist())) == 3
    assert g["e5a_out"].size == 4 * int(g["e5a_vlen"]) and int(g["e5a_vlen"]) <= 16384 and len(g["e5a_prn"]) == 2
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "siggen.npz")) < 400 * 1024
    for tag in ("gps", "e5a"):
        assert 0.0 < float(g[f"{tag}_ref_vs_model_max"]) < 0.05     # a phase error, not a structural one (the amplitudes sum to 3 and 4)


@pytest.mark.parametrize("tag", ["gps", "e5a"])
def test_model_reproduces_the_reference_block(golden, tag):
    g = golden
    sats = built_satellites(g, tag)
    ref = g[f"{tag}_out"].astype(np.complex128)
    err = np.abs(ref - R.model(sats, float(g[f"{tag}_fs"]), 0, ref.size))
    bar = float(g[f"{tag}_ref_vs_model_max"]) + 1e-6 * R.amplitude_sum(sats)
    print(f"{tag}: max |reference - model| = {err.max():.3e}, bar {bar:.3e}")
    assert err.max() <= bar
    # and in pieces that start anywhere: the model is a function of the absolute index (float64 phases of up to 100 rad: 1e-14 apart at most)
    fs = float(g[f"{tag}_fs"])
    for n0, n in ((1, 7), (3999, 4002), (ref.size - 5, 5)):
        assert np.abs(R.model(sats, fs, n0, n) - R.model(sats, fs, 0, n0 + n)[n0:]).max() < 1e-11


@pytest.mark.parametrize("tag", ["gps", "e5a"])
def test_builders_reproduce_the_fixture_tables_exactly(golden, tag):
    g = golden
    tabs = fixture_tables(g, tag)
    L = 1023 if tag == "gps" else 10230
    for scaled in (False, True):
        sats = built_satellites(g, tag, scaled)
        for s, sat in enumerate(sats):
            want = tabs[s]
            if scaled:   # complex<float> *= float (sg.cc:184, :230): each part times the scale
                want = (want.real * g[f"{tag}_scale"][s] + 1j * (want.imag * g[f"{tag}_scale"][s])).astype(np.complex64)
            table = sat.table_a if sat.table_b is None else (sat.table_a + sat.table_b).astype(np.complex64)
            assert table.dtype == np.complex64 and np.array_equal(table, want), (tag, s, scaled)
            if sat.table_b is not None:   # A = (Re, 0), B = (0, Im)
                assert not sat.table_a.imag.any() and not sat.table_b.real.any()
            assert sat.period == int(g[f"{tag}_vlen"])
            assert sat.delay_samples == (int(g[f"{tag}_delay_chips"][s]) % L) * sat.period // L
            if tag == "e5a":
                assert np.array_equal(sat.signs_a, g["e5a_signs_a"][s]) and np.array_equal(sat.signs_b, g["e5a_signs_b"][s])
            else:
                assert np.array_equal(sat.signs_a, g["gps_signs_a"][s])


def test_cn0_scale_is_the_reference_expression_in_float32(golden):
    from gnss_sdr_amd.signal_generator import cn0_scale
    g = golden
    for tag, two in (("gps", False), ("e5a", True)):
        for s, cn0 in enumerate(g[f"{tag}_cn0_db"]):
            got = cn0_scale(float(cn0), float(g[f"{tag}_fs"]) / 2.0, two)
            assert got.dtype == np.float32 and got == g[f"{tag}_scale"][s], (tag, s, got, g[f"{tag}_scale"][s])
