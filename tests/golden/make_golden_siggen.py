"""Mint tests/golden/siggen.npz: the output of the reference's own signal generator block
(src/algorithms/signal_generator/gnuradio_blocks/signal_generator_c.cc = sg.cc) with data_flag = false and noise_flag = false, which is deterministic,
for two cases:

  gps   GPS L1 C/A, PRN 1 / 10 / 25 at 4 Msps, delays 0 / 600 / 1022 chips, Doppler -3250 / 750 / +4999 Hz, C/N0 44 / 40 / 47.5 dB-Hz:
        3 consecutive vectors of 4 000 samples
  e5a   Galileo E5a, PRN 2 / 19 at 5 Msps (vector_length 5 000), delays 0 / 7000 chips, delay_sec 1, Doppler 1234.5 / -2750 Hz, C/N0 45 / 41:
        4 consecutive vectors

The block is compiled from the reference tree in a temporary directory, with the replica generators under src/algorithms/libs/, against the GNU
Radio stand-ins of tests/host/mock_gnuradio and oracle/shim.  Two things those lack are written into the temporary directory: the
gnuradio::get_initial_sptr helper (sg.cc:48) and the volk_gnsssdr_s32f_sincos_32fc dispatcher, bound to the reference kernel header's `_generic`
as oracle/ref_kernels.c binds it.  Nothing compiled stays.  No test runs this script: tests/test_siggen_reference.py and tests/test_siggen_gpu.py
read what it wrote.

Beside the block's outputs (complex64) the file holds, per case and satellite: the table the same public replica function gives for the block's
chip shift (+-1 chips as int8 I, Q: what the block holds with noise_flag false); `scale`, the float32 factor sg.cc:184 / :230 would multiply it by
with noise_flag true; the sign sequences the block applied (all +1 for GPS; for E5a entry k is what holds after k sign boundaries: entry 0 the
initial values of sg.cc:110-111, entry k >= 1 secondary chip (k - 1 + delay_sec) mod length, sg.cc:439-440); for E5a also the 10 230 primary chips
('5X': I in the real part, Q in the imaginary) and the secondary codes, as data; and ref_vs_model_max, the largest |reference - float64 model|
(tests/siggen_reference.py) over the case: the reference's own float32 phase accumulation (sg.cc:350-354), which sets a bar of the GPU tests.
The initial pilot sign of sg.cc:111 indexes the NEXT PRN's secondary code; the script refuses PRNs for which that differs from the PRN's own
chip 0, so that the sign sequences are the ones the table builder gives.

    python tests/golden/make_golden_siggen.py /path/to/gnss-sdr"""
import os
import subprocess
import sys
import tempfile
from types import SimpleNamespace

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))

GPS = dict(fs=4000000, vlen=4000, nvec=3, prn=[1, 10, 25], cn0=[44.0, 40.0, 47.5], doppler=[-3250.0, 750.0, 4999.0], delay_chips=[0, 600, 1022],
           delay_sec=[0, 0, 0])
E5A = dict(fs=5000000, vlen=5000, nvec=4, prn=[2, 19], cn0=[45.0, 41.0], doppler=[1234.5, -2750.0], delay_chips=[0, 7000], delay_sec=[1, 1])

STANDIN_H = r"""
#pragma once
#include <memory>
namespace gnuradio
{
template <class T>
std::shared_ptr<T> get_initial_sptr(T* p) { return std::shared_ptr<T>(p); }
}  // namespace gnuradio
"""

STANDIN_C = r"""
#define LV_HAVE_GENERIC 1
#include <volk_gnsssdr/volk_gnsssdr.h>
#include "volk_gnsssdr_s32f_sincos_32fc.h"
void volk_gnsssdr_s32f_sincos_32fc(lv_32fc_t* out, const float phase_inc, float* phase, unsigned int n)
{
    volk_gnsssdr_s32f_sincos_32fc_generic(out, phase_inc, phase, n);
}
"""

DRIVER = r"""
#include "signal_generator_c.h"
#include "Galileo_E5a.h"
#include "galileo_e5_signal_replica.h"
#include "gps_sdr_signal_replica.h"
#include <array>
#include <cmath>
#include <complex>
#include <cstdio>
#include <string>
#include <vector>

static void dump(const std::string& path, const void* p, size_t bytes)
{
    FILE* f = std::fopen(path.c_str(), "wb");
    std::fwrite(p, 1, bytes, f);
    std::fclose(f);
}

static std::vector<gr_complex> run(const std::vector<std::string>& signal, const std::vector<std::string>& system, const std::vector<unsigned int>& prn,
    const std::vector<float>& cn0, const std::vector<float>& doppler, const std::vector<unsigned int>& delay_chips, const std::vector<unsigned int>& delay_sec,
    unsigned int fs, unsigned int vlen, int nvec)
{
    auto blk = signal_make_generator_c(signal, system, prn, cn0, doppler, delay_chips, delay_sec, false, false, fs, vlen, 1.0F);
    std::vector<gr_complex> out(static_cast<size_t>(vlen) * nvec);
    gr_vector_int ninput;
    gr_vector_const_void_star ins;
    for (int v = 0; v < nvec; v++)
        {
            gr_vector_void_star outs{out.data() + static_cast<size_t>(v) * vlen};
            if (blk->general_work(1, ninput, ins, outs) != 1) std::exit(3);
        }
    return out;
}

int main(int, char** argv)
{
    const std::string dir = argv[1];
    {
        const unsigned int fs = @GPS_FS@, vlen = @GPS_VLEN@;
        const std::vector<unsigned int> prn{@GPS_PRN@}, delay_chips{@GPS_DELAY@}, delay_sec{@GPS_DSEC@};
        const std::vector<float> cn0{@GPS_CN0@}, doppler{@GPS_DOPPLER@};
        const size_t S = prn.size();
        auto out = run(std::vector<std::string>(S, "1C"), std::vector<std::string>(S, "G"), prn, cn0, doppler, delay_chips, delay_sec, fs, vlen, @GPS_NVEC@);
        dump(dir + "/gps_out.bin", out.data(), out.size() * sizeof(gr_complex));
        std::vector<gr_complex> tab(S * vlen);
        std::vector<float> scale(S);
        const float bw = 1.0F * static_cast<float>(fs) / 2.0F;  // BW_BB_ (sg.cc:75)
        for (size_t s = 0; s < S; s++)
            {
                std::array<gr_complex, 64000> code{};
                gps_l1_ca_code_gen_complex_sampled(code, prn[s], fs, 1023 - delay_chips[s]);
                for (unsigned int i = 0; i < vlen; i++) tab[s * vlen + i] = code[i];
                scale[s] = std::sqrt(std::pow(10.0F, cn0[s] / 10.0F) / bw);  // (sg.cc:184)
            }
        dump(dir + "/gps_tab.bin", tab.data(), tab.size() * sizeof(gr_complex));
        dump(dir + "/gps_scale.bin", scale.data(), scale.size() * sizeof(float));
    }
    {
        const unsigned int fs = @E5A_FS@, vlen = @E5A_VLEN@;
        const std::vector<unsigned int> prn{@E5A_PRN@}, delay_chips{@E5A_DELAY@}, delay_sec{@E5A_DSEC@};
        const std::vector<float> cn0{@E5A_CN0@}, doppler{@E5A_DOPPLER@};
        const size_t S = prn.size();
        auto out = run(std::vector<std::string>(S, "5X"), std::vector<std::string>(S, "E"), prn, cn0, doppler, delay_chips, delay_sec, fs, vlen, @E5A_NVEC@);
        dump(dir + "/e5a_out.bin", out.data(), out.size() * sizeof(gr_complex));
        std::vector<gr_complex> tab(S * vlen), prim(S * 10230);
        std::vector<float> scale(S);
        std::vector<signed char> sec_i(20), sec_q(S * 100), q_next0(S);
        const float bw = 1.0F * static_cast<float>(fs) / 2.0F;
        const std::array<char, 3> sig = {{'5', 'X', '\0'}};
        for (int i = 0; i < 20; i++) sec_i[i] = GALILEO_E5A_I_SECONDARY_CODE[i] == '0' ? 1 : -1;
        for (size_t s = 0; s < S; s++)
            {
                std::vector<gr_complex> code(vlen);
                galileo_e5_a_code_gen_complex_sampled(code, prn[s], sig, fs, 10230 - delay_chips[s]);
                for (unsigned int i = 0; i < vlen; i++) tab[s * vlen + i] = code[i];
                std::vector<gr_complex> p(10230);
                galileo_e5_a_code_gen_complex_primary(p, prn[s], sig);
                for (int i = 0; i < 10230; i++) prim[s * 10230 + i] = p[i];
                scale[s] = std::sqrt(std::pow(10.0F, cn0[s] / 10.0F) / bw / 2.0F);  // (sg.cc:230)
                for (int i = 0; i < 100; i++) sec_q[s * 100 + i] = GALILEO_E5A_Q_SECONDARY_CODE[prn[s] - 1][i] == '0' ? 1 : -1;
                q_next0[s] = GALILEO_E5A_Q_SECONDARY_CODE[prn[s]][0] == '0' ? 1 : -1;  // (sg.cc:111)
            }
        dump(dir + "/e5a_tab.bin", tab.data(), tab.size() * sizeof(gr_complex));
        dump(dir + "/e5a_prim.bin", prim.data(), prim.size() * sizeof(gr_complex));
        dump(dir + "/e5a_scale.bin", scale.data(), scale.size() * sizeof(float));
        dump(dir + "/e5a_sec_i.bin", sec_i.data(), sec_i.size());
        dump(dir + "/e5a_sec_q.bin", sec_q.data(), sec_q.size());
        dump(dir + "/e5a_q_next0.bin", q_next0.data(), q_next0.size());
    }
    return 0;
}
"""


def _driver_text() -> str:
    def lst(v, suffix=""):
        return ", ".join(f"{x!r}{suffix}" for x in v)
    text = DRIVER
    for tag, c in (("GPS", GPS), ("E5A", E5A)):
        for key, val in (("FS", str(c["fs"])), ("VLEN", str(c["vlen"])), ("NVEC", str(c["nvec"])), ("PRN", lst(c["prn"], "u")),
                         ("DELAY", lst(c["delay_chips"], "u")), ("DSEC", lst(c["delay_sec"], "u")), ("CN0", lst(c["cn0"], "F")),
                         ("DOPPLER", lst(c["doppler"], "F"))):
            text = text.replace(f"@{tag}_{key}@", val)
    return text


def _iq8(tab: np.ndarray) -> np.ndarray:
    """+-1 / 0 complex chips -> int8 [..., 2], exactly"""
    iq = np.stack([tab.real, tab.imag], axis=-1)
    out = iq.astype(np.int8)
    assert np.array_equal(out.astype(np.float32), iq)
    return out


def _complex(iq8: np.ndarray) -> np.ndarray:
    return (iq8[..., 0].astype(np.float32) + 1j * iq8[..., 1].astype(np.float32)).astype(np.complex64)


def used_signs(sec: np.ndarray, delay_sec: int, first: int, length: int = 100) -> np.ndarray:
    """entry k = the sign the block holds after k boundaries (sg.cc:110-111, :439-440)"""
    k = np.arange(length)
    s = np.asarray(sec, np.int8)[(k - 1 + delay_sec) % len(sec)]
    s[0] = first
    return s.astype(np.int8)


def main(reference):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import siggen_reference as R
    src = os.path.join(reference, "src")
    libs = os.path.join(src, "algorithms", "libs")
    volk = os.path.join(libs, "volk_gnsssdr_module", "volk_gnsssdr")
    blk = os.path.join(src, "algorithms", "signal_generator", "gnuradio_blocks")
    inc = ["-I" + p for p in (os.path.join(ROOT, "tests", "host", "mock_gnuradio"), os.path.join(ROOT, "oracle", "shim"), os.path.join(volk, "include"),
                              os.path.join(volk, "kernels", "volk_gnsssdr"), os.path.join(libs, "gsl", "include"), libs,
                              os.path.join(src, "core", "system_parameters"), os.path.join(src, "core", "interfaces"), blk)]
    fp = ["-O2", "-ffp-contract=off", "-fcx-limited-range", "-fno-fast-math"]   # the oracle's pinned floating-point environment (oracle/Makefile)
    with tempfile.TemporaryDirectory() as tmp:
        for name, text in (("siggen_standins.h", STANDIN_H), ("siggen_standins.c", STANDIN_C), ("driver.cc", _driver_text())):
            with open(os.path.join(tmp, name), "w") as f:
                f.write(text)
        subprocess.run(["gcc"] + fp + ["-std=gnu11", "-Wno-unused-function"] + inc + ["-c", os.path.join(tmp, "siggen_standins.c"), "-o",
                       os.path.join(tmp, "siggen_standins.o")], check=True)
        exe = os.path.join(tmp, "mint")
        sources = [os.path.join(blk, "signal_generator_c.cc")] + [os.path.join(libs, n + ".cc") for n in (
            "gnss_signal_replica", "gps_sdr_signal_replica", "galileo_e1_signal_replica", "galileo_e5_signal_replica", "galileo_e6_signal_replica",
            "glonass_l1_signal_replica")]
        subprocess.run(["g++"] + fp + ["-std=c++20", "-DHAS_STD_SPAN=1", "-DGNURADIO_USES_STD_POINTERS=1", "-DUSE_GLOG_AND_GFLAGS=1", "-w", "-include",
                       os.path.join(tmp, "siggen_standins.h")] + inc + ["-o", exe, os.path.join(tmp, "driver.cc")] + sources +
                       [os.path.join(tmp, "siggen_standins.o"), "-lm", "-lpthread"], check=True)
        subprocess.run([exe, tmp], check=True)

        def raw(name, dtype):
            return np.fromfile(os.path.join(tmp, name), dtype)
        out = {}
        for tag, c in (("gps", GPS), ("e5a", E5A)):
            S = len(c["prn"])
            tabs = raw(f"{tag}_tab.bin", np.complex64).reshape(S, c["vlen"])
            out[f"{tag}_out"] = raw(f"{tag}_out.bin", np.complex64)
            out[f"{tag}_tables_iq"] = _iq8(tabs)
            out[f"{tag}_scale"] = raw(f"{tag}_scale.bin", np.float32)
            for key in ("fs", "vlen", "nvec", "prn", "delay_chips", "delay_sec"):
                out[f"{tag}_{key}"] = np.asarray(c[key], np.int64)
            out[f"{tag}_cn0_db"] = np.asarray(c["cn0"], np.float32)
            out[f"{tag}_doppler_hz"] = np.asarray(c["doppler"], np.float32)
        S = len(E5A["prn"])
        sec_i, sec_q, q_next0 = raw("e5a_sec_i.bin", np.int8), raw("e5a_sec_q.bin", np.int8).reshape(S, 100), raw("e5a_q_next0.bin", np.int8)
        assert np.array_equal(q_next0, sec_q[:, 0]), ("sg.cc:111 starts these PRNs on another sign than their own secondary chip 0", q_next0, sec_q[:, 0])
        out["e5a_primary_iq"] = _iq8(raw("e5a_prim.bin", np.complex64).reshape(S, 10230))
        out["e5a_secondary_i"], out["e5a_secondary_q"] = sec_i, sec_q
        out["gps_signs_a"] = np.ones((len(GPS["prn"]), 1), np.int8)
        out["e5a_signs_a"] = np.stack([used_signs(sec_i, ds, sec_i[0]) for ds in E5A["delay_sec"]])
        out["e5a_signs_b"] = np.stack([used_signs(sec_q[s], E5A["delay_sec"][s], q_next0[s]) for s in range(S)])
    # the float64 model of the same scenario, from the stored tables: what the reference's float32 phase accumulation costs
    for tag, c in (("gps", GPS), ("e5a", E5A)):
        sats = []
        for s in range(len(c["prn"])):
            t = _complex(out[f"{tag}_tables_iq"][s])
            L = 1023 if tag == "gps" else 10230
            delay = ((c["delay_chips"][s] % L) * c["vlen"]) // L   # (sg.cc:360, :425)
            if tag == "gps":
                a, b, sa, sb = t, None, out["gps_signs_a"][s], np.ones(1, np.int8)
            else:
                a, b = t.real.astype(np.complex64), (1j * t.imag).astype(np.complex64)
                sa, sb = out["e5a_signs_a"][s], out["e5a_signs_b"][s]
            sats.append(SimpleNamespace(table_a=a, table_b=b, delay_samples=delay, signs_a=sa, signs_b=sb,
                                        doppler_hz=float(np.float32(c["doppler"][s])), start_phase_rad=0.0, carrier_offset_hz=0.0))
        ref = out[f"{tag}_out"].astype(np.complex128)
        out[f"{tag}_ref_vs_model_max"] = np.float64(np.abs(ref - R.model(sats, float(c["fs"]), 0, ref.size)).max())
        print(tag, "ref_vs_model_max", out[f"{tag}_ref_vs_model_max"], "amplitudes", R.amplitude_sum(sats))
    path = os.path.join(HERE, "siggen.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
