// Test helper (tests/test_exact_sum_claims.py): opensmile_amd/csrc/lld_device.hpp's float quotient helpers compiled for the HOST
// (hipcc, host side only), applied to a table of boundary values. Prints one line per value:
//   bits  needs_division(any sign)  needs_division(never negative)  sequence_equals_division(for every divisor given)
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../opensmile_amd/csrc/lld_device.hpp"

int main(int argc, char **argv) {
  int ndiv = 0;
  float divs[64];
  for (int k = 1; k < argc && argv[k][0] != '-'; ++k) divs[ndiv++] = strtof(argv[k], nullptr);
  for (int k = ndiv + 2; k < argc; ++k) {                 // after the "-": bit patterns in hex
    const uint32_t u = (uint32_t)strtoul(argv[k], nullptr, 16);
    float a;
    memcpy(&a, &u, 4);
    bool seq_ok = true;
    for (int d = 0; d < ndiv; ++d) {
      const float b = divs[d], q = a / b, s = smilehip::div_markstein(a, b, 1.0f / b);
      uint32_t qb, sb;
      memcpy(&qb, &q, 4); memcpy(&sb, &s, 4);
      seq_ok = seq_ok && (qb == sb || (q != q && s != s));
    }
    printf("%08x %d %d %d\n", u, (int)smilehip::div_needs_division(a), (int)smilehip::div_needs_division_nonneg(a), (int)seq_ok);
  }
  return 0;
}
