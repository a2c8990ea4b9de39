// mse_exact.h -- cheap forms of two quotients the step evaluates in fp64, each proven equal to the reference's literal
// expression over the range where it is used.  Shared by the kernels (mse_device.h), the host-side
// proof at mse_create (compile_config, mse_tables.h) and the exhaustive CPU proof (tests/test_exact_int_forms.py,
// which compiles this header on the host).
//
//   purity  round(tru / total, 2) in hundredths = rint(fl(fl(tru / total) * 100)): exact integer rounding of
//           100 tru / total from an f32 reciprocal estimate; exact ties and totals above kPurityExactMax take the
//           literal form
//   ratio   t / D for a launch-constant D: q = t * (1/D) plus one fma correction; the host proves it equal to the
//           literal division for every t the launch can meet, and the kernel keeps the division beyond that
#pragma once

#include <math.h>
#include <stdint.h>

#include "mse_policy_stream.h" // MSE_HD

namespace mse {

// largest container total for which purity_quotient is proven exact (the proof covers every 1 <= tru <= total and
// every f32 reciprocal within one ulp of 1 / (2 total), v_rcp_f32's documented accuracy)
constexpr uint32_t kPurityExactMax = 8192;

// the reference's expression (env_super.py:754, 785-789)
MSE_HD int purity_literal(int tru, int total)
{
    return (int)rint(((double)tru / (double)total) * 100.0);
}

// 1 / (2 total) in f32: v_rcp_f32 on the device (1 ulp); the host proof tries both neighbours as well
MSE_HD float purity_rcp(uint32_t total)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_rcpf((float)(total << 1));
#else
    return 1.0f / (float)(total << 1);
#endif
}

// round-half-up of 100 tru / total = floor(N / D) with N = 200 tru + total, D = 2 total (both < 2^24 for
// total <= kPurityExactMax).  N / D <= 100.5, and the f32 estimate N * rcp is within 1.6e-5 of it; the offset
// 2^-15 puts the estimate strictly above N / D and, when N / D is not an integer, below its ceiling (which is at
// least 1 / D >= 6.1e-5 away), so truncation gives floor(N / D) without a fix-up.  tie: N / D is an integer, i.e.
// 100 tru / total lies exactly halfway between two integers, where numpy's result depends on the rounding of the
// fp64 quotient (61 of the 2 640 ties up to 2 048 differ from half-even): the caller takes the literal form there.
MSE_HD uint32_t purity_quotient(uint32_t tru, uint32_t total, float rcp, bool &tie)
{
    const uint32_t N = 200u * (tru & 0xFFFFFFu) + total;
    const uint32_t D = total << 1;
    const uint32_t q = (uint32_t)fmaf((float)N, rcp, 0x1p-15f);
    tie = (q & 0xFFFFFFu) * (D & 0xFFFFFFu) == N;
    return q;
}

// t / D as t * (1/D) with one correction step (the residual t - q D is exact in one fma)
MSE_HD double ratio_by_reciprocal(int t, double den, double inv)
{
    const double x = (double)t;
    const double q = x * inv;
    const double r = fma(-q, den, x);
    return fma(r, inv, q);
}

// host side: the largest t_max <= limit such that ratio_by_reciprocal equals the literal t / den for every t in
// [0, t_max] (-1 if not even t = 0 does)
static inline int ratio_exact_upto(double den, double inv, int limit)
{
    for (int t = 0; t <= limit; ++t)
        if (ratio_by_reciprocal(t, den, inv) != (double)t / den) return t - 1;
    return limit;
}

} // namespace mse
