// mse_lookahead_seed.h -- the seed of a lookahead fork's fresh streams (mse_lookahead with streams = 1).
//
// One 63-bit seed per (lookahead seed, global env index, sample); the candidate action is NOT part of the key, so the
// candidates of one env and sample see the same draws.  With mix(z) the splitmix64 finaliser
//     mix(z):  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;  z = (z ^ (z >> 27)) * 0x94D049BB133111EB;  return z ^ (z >> 31)
// and all arithmetic modulo 2^64,
//     a = mix(lookahead_seed + 0x9E3779B97F4A7C15)
//     b = mix(a ^ env_index)
//     c = mix(b + ((uint64_t)sample + 1) * 0x9E3779B97F4A7C15)
//     seed = c >> 1
// The shift keeps the seed below 2^63: it is handed to mse_reset's seeding (np.random.default_rng(seed + 99 | + 4 | + 3)),
// whose callers carry seeds as signed 64-bit integers, and seed + 99 does not wrap.  mix is a bijection, so for one
// lookahead seed two (index, sample) pairs collide only where the 64-bit hashes do.  The kernel (mse_lib.hip,
// k_lookahead) and the host entry point (mse_lookahead_stream_seed) run this one function, and
// tests/test_lookahead_cpu.py restates it in numpy.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define MSE_LA_HD __host__ __device__ __forceinline__
#else
#define MSE_LA_HD static inline
#endif

MSE_LA_HD uint64_t mse_lookahead_mix(uint64_t z)
{
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

MSE_LA_HD uint64_t mse_lookahead_seed_of(uint64_t lookahead_seed, uint64_t env_index, uint32_t sample)
{
    const uint64_t a = mse_lookahead_mix(lookahead_seed + 0x9E3779B97F4A7C15ull);
    const uint64_t b = mse_lookahead_mix(a ^ env_index);
    const uint64_t c = mse_lookahead_mix(b + ((uint64_t)sample + 1ull) * 0x9E3779B97F4A7C15ull);
    return c >> 1;
}
