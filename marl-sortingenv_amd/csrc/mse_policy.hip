// Batched forward of the reference's actor-critic policy with masked categorical sampling, on the matrix cores:
// the standalone launch (mse_policy_forward).  The network, its MFMA layout and the sampling rule live in
// mse_policy_device.h (one device function per 32-env tile, shared with the fused learned-policy rollout kernel of
// mse_lib.hip); this file holds the kernel that feeds it from observation / mask tensors, the packing of
// torch.nn.Linear weights into MFMA operand order on the host and on the device (one arithmetic: mse_policy_pack.h),
// and the C ABI.  gfx950 only.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "mse.h"
#include "mse_host.h"
#include "mse_policy_device.h"
#include "mse_policy_pack.h"
#include "mse_policy_stream.h"

namespace {

using namespace msep;

struct PolicyArgs {
    long long n;
    long long index_offset;
    int d_in, n_act;
    int deterministic;
    unsigned long long seed, t;
};

// blob: the weights packed by pack_weights() below.  One wave per tile of 32 envs, grid-stride over the tiles.
template <int NR, bool F16X3>
__global__ __launch_bounds__(512) void k_policy_mlp(PolicyArgs P, const float *__restrict__ blob,
                                                    const float *__restrict__ obs, const uint8_t *__restrict__ mask,
                                                    int *__restrict__ action_out, float *__restrict__ logp_out,
                                                    float *__restrict__ value_out, float *__restrict__ logits_out)
{
    const int lane = threadIdx.x & 63, h = lane >> 5, j = lane & 31;
    // the packed weights are copied to LDS once per workgroup and read from there layer by layer (16-byte reads):
    // held in registers they would cost a wave ~100 VGPRs and every wave its own trip through L2
    extern __shared__ float wlds[];
    msep_copy_image(wlds, blob, F16X3, threadIdx.x, blockDim.x);
    __syncthreads();
    lds_f4 wl = (lds_f4)(__attribute__((address_space(3))) float *)wlds;
    const int D = P.d_in, A = P.n_act;
    const long long n_tiles = (P.n + kTile - 1) / kTile;
    const long long wave = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const long long n_waves = (long long)gridDim.x * (blockDim.x >> 6);
    for (long long tile = wave; tile < n_tiles; tile += n_waves) {
        const long long env = tile * kTile + j;
        const bool valid = env < P.n;
        const long long env_c = valid ? env : 0; // clamp: loads of padding lanes stay in bounds, results unused
        float x[16];
#pragma unroll
        for (int s = 0; s < 16; ++s) { // unconditional loads at clamped indices, then a select: no exec-mask regions
            const int k_in = 2 * s + h;
            const float v = obs[env_c * D + (k_in < D ? k_in : 0)];
            x[s] = k_in < D ? v : 0.0f;
        }
        uint32_t legal = 0; // bit r: the action of accumulator register r exists and may be taken
#pragma unroll
        for (int r = 0; r < NR; ++r) {
            const int a = row_of(r, h);
            const bool ok = a < A && (mask == nullptr || mask[env_c * A + (a < A ? a : 0)] != 0);
            legal |= (ok ? 1u : 0u) << r;
        }
        const uint32_t word = mse_policy_word(mse_policy_key(P.seed, (uint64_t)(P.index_offset + env)), P.t);
        float lgm[NR];
        const TileOut o = policy_tile<NR, F16X3>(wl, lane, x, A, legal, P.deterministic != 0, word, lgm);
        if (logits_out != nullptr) { // wave-uniform
#pragma unroll
            for (int r = 0; r < NR; ++r)
                if (row_of(r, h) < A && valid) logits_out[env * A + row_of(r, h)] = lgm[r];
        }
        if (valid && h == 0) {
            if (action_out != nullptr) action_out[env] = o.action;
            if (logp_out != nullptr) logp_out[env] = o.logp;
            if (value_out != nullptr) value_out[env] = o.value;
        }
    }
}

// torch.nn.Linear tensors (include/mse.h order) -> the image of mse_policy_device.h: A operands in the k order the
// accumulator registers impose, biases in register order, tanh folded into the weights.  mse_policy_pack.h specifies the
// image and holds its arithmetic; this is the host's walk over the cells.  From the first weight that leaves f16's range
// on, the f16 cells are left zero (their content is unspecified then).
void pack_weights(const float *w, int D, int A, float *out, bool &f16_ok)
{
    using namespace msepack;
    const Flat F = flat_offsets(D, A);
    for (int i = 0; i < kBlobFloats; ++i) out[i] = 0.0f;
    for (int i = 0; i < kOffW; ++i) out[i] = head_cell(w, F, A, i);
    f16_ok = true;
    uint16_t *h16 = reinterpret_cast<uint16_t *>(out + kOffW16); // [hi | lo][layer][chunk][lane][8]
    for (int L = 0; L < 5; ++L)
        for (int s = 0; s < 16; ++s)
            for (int lane = 0; lane < 64; ++lane) {
                const float wf = operand(w, F, D, A, L, s, lane);
                out[f32_cell(L, s, lane)] = wf;
                if (!fits_half(wf)) f16_ok = false;
                if (!f16_ok) continue;
                const HalfPair hp = split_half(wf);
                h16[f16_cell(L, s, lane)] = hp.hi;
                h16[kOperandCells + f16_cell(L, s, lane)] = hp.lo;
            }
}

std::vector<float> pack_weights(const float *w, int D, int A, bool &f16_ok)
{
    std::vector<float> out(kBlobFloats);
    pack_weights(w, D, A, out.data(), f16_ok);
    return out;
}

// The same image from flat weights in device memory, one workgroup (about 10 k cells and 32-term sums: the launch is
// latency-bound whatever its shape).  Two phases: every lane computes its cells into registers and the workgroup reduces
// "some |folded weight| >= 65 504" through LDS; only then is anything stored, so a policy pinned to f16x3 (`pinned`)
// whose new weights do not fit keeps its image, its flat copy and status[0], and status[1] says refused.  Otherwise
// the head and the f32 operands are always written, the f16 operands only when all fit, and status = {f16_ok, 0}.
// A lane owns groups of four consecutive k-steps of one operand lane: one 16-byte f32 word, 8 bytes of hi, 8 of lo.
constexpr int kPackThreads = 1024;
constexpr int kPackTrips = (msepack::kOperandGroups + kPackThreads - 1) / kPackThreads;
constexpr int kMaxWeights = 2 * (2 * kHidden * kHidden + 2 * kHidden) + kHidden * kHidden + 2 * kHidden + 1; // D = A = 32

__global__ __launch_bounds__(kPackThreads) void k_policy_pack(int D, int A, int pinned, const float *__restrict__ weights,
                                                              float *__restrict__ blob, float *__restrict__ flat_copy,
                                                              int *__restrict__ status)
{
    using namespace msepack;
    __shared__ __attribute__((aligned(16))) float w[kMaxWeights];
    __shared__ int wave_bad[kPackThreads / 64];
    const int tid = threadIdx.x;
    const Flat F = flat_offsets(D, A);
    for (int i = tid; i < F.total; i += kPackThreads) w[i] = weights[i];
    __syncthreads();
    float wf[kPackTrips][4];
    bool bad = false;
#pragma unroll
    for (int q = 0; q < kPackTrips; ++q) {
        const int g = tid + q * kPackThreads; // = (4 L + s / 4) * 64 + lane
        if (g < kOperandGroups) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                wf[q][j] = operand(w, F, D, A, g >> 8, 4 * ((g >> 6) & 3) + j, g & 63);
                bad = bad || !fits_half(wf[q][j]);
            }
        }
    }
    const int head_idx = tid - (kPackThreads - kOffW); // the last lanes, which have one operand group at most
    float head = 0.0f;
    if (head_idx >= 0) head = head_cell(w, F, A, head_idx);
    const bool wave_has_bad = __ballot(bad) != 0;
    if ((tid & 63) == 0) wave_bad[tid >> 6] = wave_has_bad ? 1 : 0;
    __syncthreads();
    int any_bad = 0;
#pragma unroll
    for (int k = 0; k < kPackThreads / 64; ++k) any_bad |= wave_bad[k];
    if (any_bad != 0 && pinned != 0) { // wave-uniform, in fact workgroup-uniform
        if (tid == 0) status[1] = 1;
        return;
    }
    for (int i = tid; i < F.total; i += kPackThreads) flat_copy[i] = w[i];
    if (head_idx >= 0) blob[head_idx] = head;
    uint2 *h16 = reinterpret_cast<uint2 *>(blob + kOffW16); // four 16-bit cells per word
#pragma unroll
    for (int q = 0; q < kPackTrips; ++q) {
        const int g = tid + q * kPackThreads;
        if (g < kOperandGroups) {
            reinterpret_cast<float4 *>(blob + kOffW)[g] = make_float4(wf[q][0], wf[q][1], wf[q][2], wf[q][3]);
            if (any_bad == 0) {
                HalfPair p[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) p[j] = split_half(wf[q][j]);
                const int at = f16_cell(g >> 8, 4 * ((g >> 6) & 3), g & 63) >> 2;
                h16[at] = make_uint2((uint32_t)p[0].hi | ((uint32_t)p[1].hi << 16), (uint32_t)p[2].hi | ((uint32_t)p[3].hi << 16));
                h16[kOperandCells / 4 + at] =
                    make_uint2((uint32_t)p[0].lo | ((uint32_t)p[1].lo << 16), (uint32_t)p[2].lo | ((uint32_t)p[3].lo << 16));
            }
        }
    }
    if (tid == 0) {
        status[0] = any_bad == 0 ? 1 : 0;
        status[1] = 0;
    }
}

// blocking read of device memory the last device repack may still be writing: behind it on its stream
bool read_behind_repack(const mse_policy *p, void *dst, const void *src, size_t bytes)
{
    hipStream_t s = static_cast<hipStream_t>(p->stream);
    return hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, s) == hipSuccess && hipStreamSynchronize(s) == hipSuccess;
}

} // namespace

extern "C" {

int64_t mse_policy_num_weights(int obs_dim, int n_actions)
{
    const int64_t H = kHidden, D = obs_dim, A = n_actions;
    return 2 * (H * D + H + H * H + H) + A * H + A + H + 1;
}

int mse_policy_create(mse_policy **out, int obs_dim, int n_actions, const float *weights_host, int device_id)
{
    if (out == nullptr || weights_host == nullptr) return mse_internal_fail(MSE_ERR_INVALID_ARGUMENT, "mse_policy_create: null argument");
    if (obs_dim < 1 || obs_dim > 32 || n_actions < 1 || n_actions > 32)
        return mse_internal_fail(MSE_ERR_UNSUPPORTED_CONFIG, "mse_policy_create: obs_dim and n_actions must be in 1..32");
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count == 0 || device_id < 0 || device_id >= count)
        return mse_internal_fail(MSE_ERR_NO_DEVICE, "mse_policy_create: no such HIP device");
    if (hipSetDevice(device_id) != hipSuccess) return mse_internal_fail(MSE_ERR_HIP, "hipSetDevice failed");
    bool f16_ok = false;
    const std::vector<float> packed = pack_weights(weights_host, obs_dim, n_actions, f16_ok);
    const int n_weights = (int)mse_policy_num_weights(obs_dim, n_actions);
    const int status0[2] = {f16_ok ? 1 : 0, 0};
    mse_policy *p = new mse_policy{obs_dim, n_actions, device_id, nullptr, packed.size(), f16_ok ? 1 : 0, 0, nullptr, nullptr, n_weights, 0, nullptr};
    if (hipMalloc(reinterpret_cast<void **>(&p->blob), p->blob_floats * sizeof(float)) != hipSuccess ||
        hipMalloc(reinterpret_cast<void **>(&p->flat), (size_t)n_weights * sizeof(float)) != hipSuccess ||
        hipMalloc(reinterpret_cast<void **>(&p->status), sizeof(status0)) != hipSuccess ||
        hipMemcpy(p->blob, packed.data(), p->blob_floats * sizeof(float), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(p->flat, weights_host, (size_t)n_weights * sizeof(float), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(p->status, status0, sizeof(status0), hipMemcpyHostToDevice) != hipSuccess) {
        if (p->blob) (void)hipFree(p->blob);
        if (p->flat) (void)hipFree(p->flat);
        if (p->status) (void)hipFree(p->status);
        delete p;
        return mse_internal_fail(MSE_ERR_HIP, "mse_policy_create: device allocation or copy failed");
    }
    *out = p;
    return MSE_OK;
}

int mse_policy_set_weights(mse_policy *p, const float *weights_host)
{
    if (p == nullptr || weights_host == nullptr) return mse_internal_fail(MSE_ERR_INVALID_ARGUMENT, "mse_policy_set_weights: null argument");
    bool f16_ok = false;
    const std::vector<float> packed = pack_weights(weights_host, p->d_in, p->n_act, f16_ok);
    if (p->precision == 2 && !f16_ok)
        return mse_internal_fail(MSE_ERR_UNSUPPORTED_CONFIG, "mse_policy_set_weights: a folded weight exceeds f16's range (65 504) and the f16x3 form was asked for");
    // blocking copy from pageable memory: hipMemcpy returns once the device image is written.  The caller keeps the
    // ordering rule of mse.h (no launch that reads this policy in flight on another stream).
    if (hipMemcpy(p->blob, packed.data(), p->blob_floats * sizeof(float), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(p->flat, weights_host, (size_t)p->n_weights * sizeof(float), hipMemcpyHostToDevice) != hipSuccess)
        return mse_internal_fail(MSE_ERR_HIP, "mse_policy_set_weights: device copy failed");
    p->f16_ok = f16_ok ? 1 : 0;
    p->pending = 0; // this image replaces whatever a device repack left: its status no longer matters
    return MSE_OK;
}

int mse_policy_set_weights_device(mse_policy *p, const float *weights_dev, void *stream)
{
    if (p == nullptr || weights_dev == nullptr)
        return mse_internal_fail(MSE_ERR_INVALID_ARGUMENT, "mse_policy_set_weights_device: null argument");
    hipLaunchKernelGGL(k_policy_pack, dim3(1), dim3(kPackThreads), 0, static_cast<hipStream_t>(stream), p->d_in, p->n_act,
                       p->precision == 2 ? 1 : 0, weights_dev, p->blob, p->flat, p->status);
    if (hipGetLastError() != hipSuccess) return mse_internal_fail(MSE_ERR_HIP, "mse_policy_set_weights_device: kernel launch failed");
    p->pending = 1;
    p->stream = stream;
    return MSE_OK;
}

int mse_policy_sync(mse_policy *p)
{
    if (p == nullptr) return mse_internal_fail(MSE_ERR_INVALID_ARGUMENT, "mse_policy_sync: null argument");
    if (!p->pending) return MSE_OK;
    int status[2] = {0, 0};
    if (!read_behind_repack(p, status, p->status, sizeof(status))) return mse_internal_fail(MSE_ERR_HIP, "mse_policy_sync: device read failed");
    p->pending = 0;
    if (status[1] != 0)
        return mse_internal_fail(MSE_ERR_UNSUPPORTED_CONFIG, "mse_policy_sync: a folded weight exceeds f16's range (65 504) and the f16x3 form was asked for; the policy keeps its previous weights");
    p->f16_ok = status[0] != 0 ? 1 : 0;
    return MSE_OK;
}

int64_t mse_policy_image_floats(void) { return kBlobFloats; }

int mse_policy_pack_host(int obs_dim, int n_actions, const float *weights_host, float *image_out, int32_t *f16_ok_out)
{
    if (weights_host == nullptr || image_out == nullptr || f16_ok_out == nullptr)
        return mse_internal_fail(MSE_ERR_INVALID_ARGUMENT, "mse_policy_pack_host: null argument");
    if (obs_dim < 1 || obs_dim > 32 || n_actions < 1 || n_actions > 32)
        return mse_internal_fail(MSE_ERR_UNSUPPORTED_CONFIG, "mse_policy_pack_host: obs_dim and n_actions must be in 1..32");
    bool f16_ok = false;
    pack_weights(weights_host, obs_dim, n_actions, image_out, f16_ok);
    *f16_ok_out = f16_ok ? 1 : 0;
    return MSE_OK;
}

int mse_policy_read_image(mse_policy *p, float *image_out_host)
{
    if (p == nullptr || image_out_host == nullptr) return mse_internal_fail(MSE_ERR_INVALID_ARGUMENT, "mse_policy_read_image: null argument");
    if (!read_behind_repack(p, image_out_host, p->blob, p->blob_floats * sizeof(float)))
        return mse_internal_fail(MSE_ERR_HIP, "mse_policy_read_image: device read failed");
    return MSE_OK;
}

int mse_policy_get_weights(mse_policy *p, float *out_host)
{
    if (p == nullptr || out_host == nullptr) return mse_internal_fail(MSE_ERR_INVALID_ARGUMENT, "mse_policy_get_weights: null argument");
    if (!read_behind_repack(p, out_host, p->flat, (size_t)p->n_weights * sizeof(float)))
        return mse_internal_fail(MSE_ERR_HIP, "mse_policy_get_weights: device read failed");
    return MSE_OK;
}

int mse_policy_set_precision(mse_policy *p, int mode)
{
    if (p == nullptr || mode < 0 || mode > 2) return mse_internal_fail(MSE_ERR_INVALID_ARGUMENT, "mse_policy_set_precision: bad argument");
    if (mode == 2 && !p->f16_ok)
        return mse_internal_fail(MSE_ERR_UNSUPPORTED_CONFIG, "mse_policy_set_precision: a folded weight exceeds f16's range (65 504)");
    p->precision = mode;
    return MSE_OK;
}

int mse_policy_precision(const mse_policy *p) { return p == nullptr ? -1 : (p->use_f16() ? 2 : 1); }

int mse_policy_destroy(mse_policy *p)
{
    if (p == nullptr) return MSE_OK;
    (void)hipFree(p->blob);
    (void)hipFree(p->flat);
    (void)hipFree(p->status);
    delete p;
    return MSE_OK;
}

int mse_policy_forward(mse_policy *p, int64_t n, int64_t index_offset, const float *obs_dev, const uint8_t *mask_dev,
                       uint64_t seed, uint64_t t, int deterministic, int32_t *action_out, float *logp_out,
                       float *value_out, float *logits_out, void *stream)
{
    if (p == nullptr || obs_dev == nullptr || n < 0) return mse_internal_fail(MSE_ERR_INVALID_ARGUMENT, "mse_policy_forward: bad argument");
    if (n == 0) return MSE_OK;
    PolicyArgs a{(long long)n, (long long)index_offset, p->d_in, p->n_act, deterministic ? 1 : 0, seed, t};
    const long long tiles = (n + kTile - 1) / kTile;
    long long blocks = (tiles + 7) / 8; // 8 waves per block = two per SIMD
    if (blocks > 512) blocks = 512;     // two workgroups per CU (21 KB of LDS each), then grid-stride over the tiles
    const int nr = regs_for_actions(p->n_act); // accumulator registers that can hold an action: 2 .. 16
#define MSE_LAUNCH_POLICY(NR, F16)                                                                                   \
    hipLaunchKernelGGL((k_policy_mlp<NR, F16>), dim3((unsigned)blocks), dim3(512), kLdsFloats * sizeof(float),       \
                       static_cast<hipStream_t>(stream), a, p->blob, obs_dev, mask_dev, action_out, logp_out,        \
                       value_out, logits_out)
    if (p->use_f16()) {
        if (nr <= 2) MSE_LAUNCH_POLICY(2, true);
        else if (nr <= 7) MSE_LAUNCH_POLICY(7, true);
        else if (nr <= 12) MSE_LAUNCH_POLICY(12, true);
        else MSE_LAUNCH_POLICY(16, true);
    } else {
        if (nr <= 2) MSE_LAUNCH_POLICY(2, false);
        else if (nr <= 7) MSE_LAUNCH_POLICY(7, false);
        else if (nr <= 12) MSE_LAUNCH_POLICY(12, false);
        else MSE_LAUNCH_POLICY(16, false);
    }
#undef MSE_LAUNCH_POLICY
    if (hipGetLastError() != hipSuccess) return mse_internal_fail(MSE_ERR_HIP, "mse_policy_forward: kernel launch failed");
    return MSE_OK;
}

} // extern "C"
