// The random stream of the training augmentation (augment.hip, include/deflow_amd.h): Philox4x32-10 with the
// standard constants (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11; the Random123 known answers are in
// tests/test_augment_cpu.py).  Counter-based: a word is a pure function of (counter, key), so nothing is stored between calls and no
// lane depends on another.  Host and device: the same text serves a stand-alone host check.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define DF_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define DF_HD inline
#endif

// ten rounds, the key bumped between rounds (nine times): ctr and key in, four words out
DF_HD void df_philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t out[4]) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1;
    c3 = (uint32_t)p0;
    c0 = n0;
    c2 = n2;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  out[0] = c0;
  out[1] = c1;
  out[2] = c2;
  out[3] = c3;
}

// a word as a uniform value in [0, 1): its top 24 bits, exact in fp32
DF_HD float df_u01(uint32_t w) { return (float)(w >> 8) * 5.9604644775390625e-8f; }

// a word as an Irwin-Hall bell: the sum of its four bytes minus its mean 510, an integer in [-510, 510] of standard deviation
// sqrt(4 (256^2 - 1) / 12) = 147.8
DF_HD float df_bell(uint32_t w) { return (float)((int)((w & 255u) + ((w >> 8) & 255u) + ((w >> 16) & 255u) + (w >> 24)) - 510); }
