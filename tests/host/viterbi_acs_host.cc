// Host build of gnss-sdr_amd/csrc/viterbi_acs.h for tests/test_viterbi_acs_host.py: a job table walked on one thread with the functions as they are,
// the way tlm_pages_kernel walks it with 64 lanes.  The carried metrics (64 floats per channel, -1e7 for a fresh decoder) and the CRC chain registers
// belong to the caller, as they belong to the handle in the library.
#include "gnss_sdr_hip.h"
#include "viterbi_acs.h"
#include <vector>

extern "C"
{
    int gsh_test_tlm_sizes(int* job_bytes, int* result_bytes)
    {
        *job_bytes = static_cast<int>(sizeof(gsh_tlm_page_job));
        *result_bytes = static_cast<int>(sizeof(gsh_tlm_page_result));
        return gsh::TLM_STATES;
    }

    // 0, or 1 + the index of the first job that fails a range check
    int gsh_test_tlm_run_jobs(int metric_mode, int n_channels, const float* symbols, uint64_t n_symbols, const gsh_tlm_page_job* jobs, int n_jobs,
        gsh_tlm_page_result* results, float* metrics, uint32_t* chain)
    {
        std::vector<uint64_t> words(gsh::TLM_MAX_STEPS);
        for (int j = 0; j < n_jobs; j++)
            {
                const gsh_tlm_page_job& job = jobs[j];
                gsh::TlmGeometry g;
                if (!gsh::tlm_geometry(job.frame_type, g) || job.channel < 0 || job.channel >= n_channels || job.symbol_offset + g.symbols > n_symbols) return 1 + j;
                uint32_t* bits = results[j].bits;
                gsh::tlm_decode_page(metric_mode, g, symbols + job.symbol_offset, (job.flags & gsh::TLM_JOB_INVERT) != 0,
                    metrics + static_cast<size_t>(job.channel) * gsh::TLM_STATES, words.data(), bits);
                bool cont, check;
                int n_bits, ok;
                gsh::tlm_crc_plan(job.flags, job.crc_bits, job.crc_check, bits, cont, n_bits, check);
                chain[job.channel] = gsh::tlm_crc_run(cont ? chain[job.channel] : 0u, bits, n_bits, check, ok);
                results[j].crc_register = chain[job.channel];
                results[j].crc_ok = ok;
            }
        return 0;
    }

    uint32_t gsh_test_tlm_crc_bytes(const uint8_t* bytes, int n)
    {
        uint32_t reg = 0;
        for (int i = 0; i < n; i++)
            for (int b = 7; b >= 0; b--) reg = gsh::tlm_crc24q_bit(reg, (bytes[i] >> b) & 1u);
        return reg;
    }

    int gsh_test_tlm_preamble_chip(int frame_type, int k) { return gsh::tlm_preamble_chip(frame_type, k); }

    int gsh_test_tlm_out_symbol(int input, int state) { return gsh::tlm_out_symbol(input, state); }
}
