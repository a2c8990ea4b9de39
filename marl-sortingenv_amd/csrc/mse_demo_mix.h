// mse_demo_mix.h -- who steps in a demonstration rollout (mse_rollout_demo): the expert or the student.
//
// One decision per (mix seed, global env index, step counter t), taken from a word of the policy stream
// (mse_policy_stream.h) under a seed of its own: the expert's action is stepped iff the word's upper 24 bits are below
// `expert_threshold`, an integer in [0, 2^24].  0: the student always steps; 2^24: the expert always steps; between
// them the expert's share is expert_threshold / 2^24 of the words.  Integers only, nothing is rounded: the kernel
// (mse_lib.hip, k_rollout_demo) and the host twin (mse_demo_who_steps_host) run this one function, and
// tests/test_demo_mixture_cpu.py restates it in numpy.
#pragma once

#include "mse_policy_stream.h"

#define MSE_DEMO_THRESHOLD_ONE (1u << 24) /* expert_threshold of beta = 1 */

// mix_key = mse_policy_key(mix_seed, global env index): constant over a launch
MSE_HD bool mse_demo_expert_steps(uint32_t mix_key, uint64_t t, uint32_t expert_threshold)
{
    return (mse_policy_word(mix_key, t) >> 8) < expert_threshold;
}
