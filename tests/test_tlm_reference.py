"""tests/tlm_reference.py (the numpy float32 restatement of the Galileo page decoder) against tests/golden/viterbi.npz, which
tests/golden/make_golden_viterbi.py minted from the reference's own Viterbi_Decoder.  All comparisons are of bits; there is no tolerance.

Reference mode (first symbol of a pair only, metrics carried from page to page) must equal the reference on EVERY page, noisy ones included, for a fresh
object per page and for one object reused over the pages.  Full mode (both symbols, every page from state 0) is the correct decoder: it recovers the
transmitted bits wherever the fixture's float64 maximum-likelihood decoder was checked to (sigma <= 0.3), and it can be compared with the reference only
where that one makes no error: on the noise-free pages."""
import numpy as np
import pytest

import tlm_reference as R


@pytest.mark.parametrize("name,frame_type", R.FIXTURE_FRAMES)
def test_fixture_holds_every_length_amplitude_and_noise_level(name, frame_type):
    z = R.fixture()
    g = R.GEOMETRY[frame_type]
    assert z[name + "__sym"].shape[1] == g["symbols"] and z[name + "__tx"].shape[1] == g["info_bits"]
    assert sorted(set(z[name + "__amp"])) == [1.0, 2500.0] and sorted(set(z[name + "__sigma"])) == [0.0, 0.3, 0.6, 1.0]
    quiet = z[name + "__sigma"] <= 0.3
    assert np.array_equal(z[name + "__ml"][quiet], z[name + "__tx"][quiet])


@pytest.mark.parametrize("name,frame_type", R.FIXTURE_FRAMES)
def test_reference_mode_equals_a_fresh_reference_object_on_every_page(name, frame_type):
    assert np.array_equal(R.fixture_decoded("reference", False)[name], R.fixture()[name + "__fresh"])


@pytest.mark.parametrize("name,frame_type", R.FIXTURE_FRAMES)
def test_reference_mode_equals_one_reused_reference_object_on_every_page(name, frame_type):
    assert np.array_equal(R.fixture_decoded("reference", True)[name], R.fixture()[name + "__reused"])


@pytest.mark.parametrize("name,frame_type", R.FIXTURE_FRAMES)
def test_full_mode_recovers_the_transmitted_bits_up_to_sigma_0p3(name, frame_type):
    z = R.fixture()
    quiet = z[name + "__sigma"] <= 0.3
    assert quiet.sum() == len(quiet) // 2
    assert np.array_equal(R.fixture_decoded("full", False)[name][quiet], z[name + "__tx"][quiet])


@pytest.mark.parametrize("name,frame_type", R.FIXTURE_FRAMES)
def test_full_mode_equals_the_reference_on_every_noise_free_page(name, frame_type):
    z = R.fixture()
    clean = z[name + "__sigma"] == 0.0
    assert set(z[name + "__amp"][clean]) == {1.0, 2500.0}
    full = R.fixture_decoded("full", False)[name][clean]
    assert np.array_equal(full, z[name + "__fresh"][clean]) and np.array_equal(full, z[name + "__reused"][clean])


def test_crc24q_known_answer():
    z = R.fixture()
    assert int(z["crc_value"][0]) == 0xCDE703 and bytes(z["crc_message"]) == b"123456789"
    assert R.crc24q(np.unpackbits(z["crc_message"])) == 0xCDE703
    # leading zero bits change nothing with a zero initial register (the reference pads to whole bytes that way)
    assert R.crc24q(np.concatenate([np.zeros(4, np.uint8), np.unpackbits(z["crc_message"])])) == 0xCDE703


def test_the_encoder_of_the_tests_round_trips():
    rng = np.random.default_rng(3)
    for ft, g in R.GEOMETRY.items():
        info = rng.integers(0, 2, g["info_bits"]).astype(np.uint8)
        for metric in ("full", "reference"):
            bits, _ = R.viterbi(R.soft_values(R.encode_page(info, ft), ft), g["info_bits"], metric)
            assert np.array_equal(bits, info)
        bits, _ = R.viterbi(R.soft_values(-R.encode_page(info, ft), ft, invert=True), g["info_bits"], "full")
        assert np.array_equal(bits, info)
