"""TEST INFRASTRUCTURE ONLY.  The test programs that compile against the reference's own headers and sources (taken from where they lie
under the reference tree) and link the checkers of oracle/_ref/: built into oracle/_ref/ beside them, only where the reference tree is present,
and they travel with oracle/_ref/ to the machine that runs the GPU tests.  Their run paths are relative ($ORIGIN), so they find libgnss_sdr_hip.so and the checkers
wherever the tree lies.  Called by __graft_entry__.build()."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "gnss-sdr_amd")
REF_OUT = os.path.join(ROOT, "oracle", "_ref")
# run paths of a program in oracle/_ref/: the engine library, the checkers beside it, liboracle.so one level up
RPATH_PKG, RPATH_REF, RPATH_ORACLE = "-Wl,-rpath,$ORIGIN/../../gnss-sdr_amd", "-Wl,-rpath,$ORIGIN", "-Wl,-rpath,$ORIGIN/.."


def reference_tree() -> str:
    """The reference tree oracle/Makefile compiles the checkers from: its REF, which the environment overrides there as here."""
    if os.environ.get("REF"):
        return os.environ["REF"]
    with open(os.path.join(ROOT, "oracle", "Makefile")) as f:
        for line in f:
            if line.split("?=")[0].strip() == "REF":
                return line.split("?=", 1)[1].strip()
    return ""


def build_adapter_test(reference: str = "") -> str:
    """The gnss-sdr adapters (gnss-sdr_amd/host/gnss_sdr_adapters/) compiled against the reference's OWN interface headers and a few of
    its sources (acq_conf.cc, in_memory_configuration.cc, string_converter.cc, the replica generators already built into
    oracle/_ref/) taken from where they lie, plus tests/host/mock_gnuradio/ for the GNU Radio runtime -> oracle/_ref/test_adapters.
    Only possible where the reference tree is present; the binary travels to the GPU box with oracle/_ref/."""
    out = os.path.join(REF_OUT, "test_adapters")
    R = os.path.join(reference or reference_tree(), "src")
    if not os.path.isdir(R):
        return out if os.path.exists(out) else ""
    import glob
    host = os.path.join(PKG, "host")
    inc = [os.path.join(ROOT, "tests", "host", "mock_gnuradio"), os.path.join(ROOT, "include"), host, os.path.join(host, "gnss_sdr_adapters")] + [
        os.path.join(R, d) for d in ("core/interfaces", "core/system_parameters", "core/receiver", "core/libs", "algorithms/libs",
                                     "algorithms/acquisition/libs", "algorithms/acquisition/gnuradio_blocks", "algorithms/channel/libs")]
    srcs = [os.path.join(ROOT, "tests", "host", "test_adapters.cc"), os.path.join(host, "hip_pcps_acquisition_core.cc"), os.path.join(host, "hip_pcps_detectors.cc"),
            os.path.join(host, "hip_acquisition_runtime.cc")]
    srcs += sorted(f for f in glob.glob(os.path.join(host, "gnss_sdr_adapters", "*.cc")) if not os.path.basename(f).startswith("dll_pll_"))
    srcs += [os.path.join(R, "algorithms/acquisition/libs/acq_conf.cc"), os.path.join(R, "core/receiver/in_memory_configuration.cc"),
             os.path.join(R, "core/libs/string_converter.cc")]
    objs = [os.path.join(ROOT, "oracle", "_ref", o) for o in ("gps_sdr_signal_replica.o", "galileo_e1_signal_replica.o", "gps_l5_signal_replica.o",
                                                               "gnss_signal_replica.o", "gps_l2c_signal_replica.o", "galileo_e5_signal_replica.o",
                                                               "beidou_b1i_signal_replica.o", "beidou_b3i_signal_replica.o", "galileo_e6_signal_replica.o",
                                                               "glonass_l1_signal_replica.o", "glonass_l2_signal_replica.o", "qzss_signal_replica.o")]
    cmd = ["g++", "-std=c++20", "-O1", "-pthread", "-DHAS_STD_SPAN=1", "-DGNURADIO_USES_STD_POINTERS=1", "-DUSE_GLOG_AND_GFLAGS=1"] + ["-I" + i for i in inc] + [
        "-o", out] + srcs + objs + ["-L" + PKG, "-lgnss_sdr_hip", "-L" + os.path.join(ROOT, "oracle", "_ref"), "-lgnsssdr_ref_acq",
                                     RPATH_PKG, RPATH_REF, "-Wl,-rpath,/opt/rocm/lib"]
    subprocess.run(cmd, check=True)
    return out


def build_tracking_adapter_test(reference: str = "") -> str:
    """The TrackingInterface adapters + GNU Radio block shell + Dll_Pll_Conf mapper (gnss-sdr_amd/host/gnss_sdr_adapters/dll_pll_*_hip.cc) and
    Hip_Tracking_Runtime compiled against the reference's own headers and tests/host/mock_gnuradio, linked with the CHECKER
    oracle/_ref/libgnsssdr_ref_trk.so (the reference's own tracking chain; also provides Dll_Pll_Conf, the flag defaults and the replica
    generators the adapters call) -> oracle/_ref/test_tracking_adapters.  Only where the reference tree is present."""
    out = os.path.join(REF_OUT, "test_tracking_adapters")
    R = os.path.join(reference or reference_tree(), "src")
    ref_so = os.path.join(ROOT, "oracle", "_ref", "libgnsssdr_ref_trk.so")
    if not os.path.isdir(R) or not os.path.exists(ref_so):
        return out if os.path.exists(out) else ""
    host = os.path.join(PKG, "host")
    ad = os.path.join(host, "gnss_sdr_adapters")
    inc = [os.path.join(ROOT, "tests", "host", "mock_gnuradio"), os.path.join(ROOT, "oracle", "shim_blocks"), os.path.join(ROOT, "oracle", "shim"),
           os.path.join(ROOT, "include"), host, ad] + [
        os.path.join(R, d) for d in ("core/interfaces", "core/system_parameters", "core/receiver", "core/libs", "algorithms/libs",
                                     "algorithms/tracking/libs", "algorithms/channel/libs",
                                     "algorithms/libs/volk_gnsssdr_module/volk_gnsssdr/include")]
    srcs = [os.path.join(ROOT, "tests", "host", "test_tracking_adapters.cc"), os.path.join(host, "hip_tracking_runtime.cc"),
            os.path.join(host, "hip_correlator_runtime.cc"), os.path.join(host, "hip_multicorrelator_real_codes.cc"),
            os.path.join(ad, "dll_pll_conf_hip.cc"), os.path.join(ad, "dll_pll_veml_tracking_hip.cc"), os.path.join(ad, "dll_pll_tracking_hip.cc")]
    cmd = ["g++", "-std=c++20", "-O1", "-pthread", "-DHAS_STD_SPAN=1", "-DGNURADIO_USES_STD_POINTERS=1", "-DUSE_GLOG_AND_GFLAGS=1",
           "-DGNURADIO_GREATER_THAN_38=1"] + ["-I" + i for i in inc] + ["-o", out] + srcs + [
        "-L" + PKG, "-lgnss_sdr_hip", "-L" + os.path.dirname(ref_so), "-lgnsssdr_ref_trk",
        RPATH_PKG, RPATH_REF, "-Wl,-rpath,/opt/rocm/lib"]
    subprocess.run(cmd, check=True)
    # the same program in front of tests/host/fake_gsh_engine.cc (CPU stand-in for the device half of the C ABI, the oracle's loop behind it): what the
    # CPU suite runs -- threads, locks, block bookkeeping, dump, TOW -- where no GPU exists.  Test infrastructure; optionally under ThreadSanitizer.
    fake = out + "_fake"
    i = cmd.index("-o")
    cmd_fake = cmd[:i] + ["-I" + os.path.join(ROOT, "oracle"), "-o", fake] + srcs + [os.path.join(ROOT, "tests", "host", "fake_gsh_engine.cc")] + [
        "-L" + os.path.join(ROOT, "oracle"), "-loracle", RPATH_ORACLE] + cmd[i + 2 + len(srcs):]
    subprocess.run(cmd_fake, check=True)
    return out


def build_channel_test(reference: str = "", tsan: bool = False) -> str:
    """oracle/_ref/test_channel: the reference's OWN Channel / ChannelFsm / channel_msg_receiver_cc (compiled in place into oracle/_ref/libgnsssdr_ref_chan.so, with the
    reference's acquisition and tracking adapters and blocks: the checker) over the HIP acquisition + tracking adapters, on tests/host/mini_flowgraph.h.  Two binaries:
    test_channel (libgnss_sdr_hip.so: the GPU box) and test_channel_fake (tests/host/fake_gsh_engine.cc in front of it: the CPU suite, ThreadSanitizer).
    Only where the reference tree is present; the binaries travel with oracle/_ref/."""
    import glob
    out = os.path.join(REF_OUT, "test_channel")
    R = os.path.join(reference or reference_tree(), "src")
    ref_so = os.path.join(ROOT, "oracle", "_ref", "libgnsssdr_ref_chan.so")
    if not os.path.isdir(R) or not os.path.exists(ref_so):
        return out if os.path.exists(out) else ""
    host = os.path.join(PKG, "host")
    ad = os.path.join(host, "gnss_sdr_adapters")
    inc = [os.path.join(ROOT, "tests", "host", "mock_gnuradio"), os.path.join(ROOT, "tests", "host"), os.path.join(ROOT, "oracle", "shim_blocks"), os.path.join(ROOT, "oracle", "shim"),
           os.path.join(ROOT, "oracle"), os.path.join(ROOT, "include"), host, ad] + [
        os.path.join(R, d) for d in ("core/interfaces", "core/system_parameters", "core/receiver", "core/libs", "algorithms/libs", "algorithms/tracking/libs",
                                     "algorithms/acquisition/libs", "algorithms/acquisition/gnuradio_blocks", "algorithms/channel/libs", "algorithms/channel/adapters",
                                     "algorithms/libs/volk_gnsssdr_module/volk_gnsssdr/include")]
    srcs = [os.path.join(ROOT, "tests", "host", "test_channel.cc")] + [os.path.join(host, f) for f in (
        "hip_tracking_runtime.cc", "hip_correlator_runtime.cc", "hip_multicorrelator_real_codes.cc", "hip_pcps_acquisition_core.cc", "hip_pcps_detectors.cc",
        "hip_acquisition_runtime.cc")] + sorted(glob.glob(os.path.join(ad, "*.cc")))
    flags = ["g++", "-std=c++20", "-O1", "-g", "-pthread", "-DHAS_STD_SPAN=1", "-DGNURADIO_USES_STD_POINTERS=1", "-DUSE_GLOG_AND_GFLAGS=1", "-DGNURADIO_GREATER_THAN_38=1",
             "-DHAS_GENERIC_LAMBDA=1", "-DPMT_USES_BOOST_ANY=0"] + (["-fsanitize=thread"] if tsan else []) + ["-I" + i for i in inc]
    link = ["-L" + PKG, "-lgnss_sdr_hip", "-L" + os.path.dirname(ref_so), "-lgnsssdr_ref_chan", RPATH_PKG, RPATH_REF, "-Wl,-rpath,/opt/rocm/lib"]
    if not tsan:
        subprocess.run(flags + ["-o", out] + srcs + link, check=True)
    fake = out + ("_fake_tsan" if tsan else "_fake")
    subprocess.run(flags + ["-o", fake] + srcs + [os.path.join(ROOT, "tests", "host", "fake_gsh_engine.cc")] +
                   ["-L" + os.path.join(ROOT, "oracle"), "-loracle", RPATH_ORACLE] + link, check=True)
    return fake if tsan else out
