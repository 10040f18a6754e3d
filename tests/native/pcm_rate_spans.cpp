// Prints what the rate matcher's launch geometry (csrc/sdrfm_pcm_rate.h) makes of one stream's call: "<span length> <spans that take outputs> <outputs>".
// Arguments: pos step n n_taps log2_phases max_step.  tests/test_pcm_rate_gpu.py asks it how many workgroups a stream's outputs spread over.
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "../../stm32f7-rtlsdr_amd/csrc/sdrfm_pcm_rate.h"

int main(int argc, char** argv) {
  if (argc != 7) return 2;
  const uint64_t pos = strtoull(argv[1], nullptr, 10), step = strtoull(argv[2], nullptr, 10), max_step = strtoull(argv[6], nullptr, 10);
  const uint32_t n = (uint32_t)strtoul(argv[3], nullptr, 10), nt = (uint32_t)strtoul(argv[4], nullptr, 10), logph = (uint32_t)strtoul(argv[5], nullptr, 10);
  const uint32_t cnt = rate_count(pos, step, n), span = rate_span_len(max_step, nt, logph);
  uint32_t busy = 0;
  for (uint32_t b = 0; b < (cnt + span - 1) / span + 1; ++b) {
    uint32_t first, count, w;
    int64_t w0;
    rate_span(pos, step, cnt, span, b, nt, &first, &count, &w0, &w);
    busy += count ? 1u : 0u;
  }
  printf("%u %u %u\n", span, busy, cnt);
  return 0;
}
