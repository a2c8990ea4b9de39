"""Host restatements the policy-head tests are held against (not a test module): the accumulator register order and
kernel selector of csrc/mse_policy_device.h / mse_policy.hip, torch.argmax's first maximum on the masked float64
logits, the constant-logit head, the sampler's inverse cdf for a uniform policy in float32 bit for bit, the weight sets
and the float64 / float32 torch evaluation of the network, and the forward checker tests/test_gpu_policy.py and
tests/test_gpu_policy_shapes.py share.  numpy and torch on the CPU only; `check_forward` is handed the device policy.

The decision rules pinned here:
  * deterministic: argmax of the masked logits, ties to the LOWEST ACTION INDEX (torch.argmax, SB3's mode());
  * sampled: inverse cdf of u = (word >> 8) 2^-24 over the softmax masses in REGISTER order - half 0's rows ascending
    (0-3, 8-11, 16-19, 24-27), then half 1's (4-7, 12-15, 20-23, 28-31) - the first register whose running sum exceeds
    u x total, where the target is clamped below the half's mass (x (1 - 2^-23)) so that rounding never carries a draw
    past the last register with mass;
  * a mask row with no legal action is the uniform distribution over the A actions (MaskableCategorical: every logit
    -1e8), deterministic action 0.
"""
import numpy as np

from tests import policy_stream as ps

LOGIT_TOL, LOGP_TOL = 2e-5, 1e-4
# the f16x3 form on the saturating weight set (pre-activations up to ~40): it carries 22-bit operand splits, not f32's
# 24 bits; measured 2.7e-5 against float64 (the f32 form 1.8e-5, torch's own fp32 1.1e-5)
SATURATING_F16X3_LOGIT_TOL = 4e-5

HUGE_NEG_BITS = 0xCCBEBC20  # float32(-1e8), sb3_contrib's HUGE_NEG: what an illegal action's logit reads, exactly
KERNEL_REGS = (2, 7, 12, 16)  # the NR instantiations of k_policy_mlp

# Global env indices whose draw under (seed 77, t 3) is u = 0 (word >> 8 == 0) and u = 1 - 2^-24 (word >> 8 ==
# 0xFFFFFF): found by scanning policy_stream.word(77, idx, 3) over idx < 2^27; the tests re-derive each word.
EXTREME_SEED, EXTREME_T = 77, 3
U_ZERO_INDICES = (19400928, 116229966)
U_MAX_INDICES = (3398609, 7137463, 11543906, 17146233)


def row_of(r, h):
    return (r & 3) + 8 * (r >> 2) + 4 * h


def regs_for_actions(A):
    """Accumulator registers that can hold an action row < A in either half."""
    return max(r + 1 for r in range(16) for h in (0, 1) if row_of(r, h) < A)


def kernel_regs(A):
    """The NR of the k_policy_mlp instantiation mse_policy_forward launches for A actions."""
    return next(nr for nr in KERNEL_REGS if regs_for_actions(A) <= nr)


def register_order(A):
    """The actions in the order the sampler walks them: half 0's registers ascending, then half 1's, rows < A."""
    return [a for h in (0, 1) for r in range(16) for a in [row_of(r, h)] if a < A]


def half_of(a):
    return (a >> 2) & 1


def first_argmax(logits64, mask=None):
    """torch.argmax (the first maximum) of the float64 logits with illegal actions at -1e8 -> int64 numpy [N]."""
    import torch

    lg = torch.tensor(np.array(logits64, dtype=np.float64))
    if mask is not None:
        lg[~torch.as_tensor(np.asarray(mask).astype(bool))] = -1e8
    return lg.argmax(dim=1).numpy()


# ---- weight sets and the network in torch ----------------------------------------------------------------------------
def weights(obs_dim, n_actions, seed):
    import torch

    from marl_sortingenv_amd.policy import SB3_KEYS, _shapes

    g = torch.Generator().manual_seed(seed)
    return {k: (torch.randn(s, generator=g) * (0.5 if len(s) == 2 else 0.1)).float()
            for k, s in zip(SB3_KEYS, _shapes(obs_dim, n_actions))}


def saturating_weights(obs_dim, n_actions, seed):
    """Hidden layers at 8x SB3's initial scale (pre-activations of several units: tanh saturates, the folded tanh's
    exp2 overflows) and the action head at gain 3 (logits reach tens: a softmax dominated by one action)."""
    import torch

    from marl_sortingenv_amd.policy import SB3_KEYS, _shapes

    g = torch.Generator().manual_seed(seed)
    w = {}
    for k, s in zip(SB3_KEYS, _shapes(obs_dim, n_actions)):
        if len(s) == 1:
            w[k] = (torch.randn(s, generator=g) * 0.1).float()
        else:
            gain = 3.0 if k == "action_net.weight" else (1.0 if k == "value_net.weight" else 8.0 * 2.0 ** 0.5)
            w[k] = (torch.randn(s, generator=g) * gain / s[1] ** 0.5).float()
    return w


def constant_head_weights(obs_dim, n_actions, bias, seed=0):
    """The constant-logit head: action_net.weight all zero, action_net.bias = `bias` (length A); hidden layers and the
    critic random.  The folded head bias is then the bias itself (b' = b + W 1 with W = 0) and every MFMA of the head
    adds 0, so the device logits are the bias bit for bit in both product forms (asserted by `assert_constant_head`)."""
    import torch

    w = weights(obs_dim, n_actions, seed)
    w["action_net.weight"] = torch.zeros_like(w["action_net.weight"])
    w["action_net.bias"] = torch.as_tensor(np.asarray(bias, dtype=np.float32)).clone().reshape(n_actions)
    return w


def assert_constant_head(logits_dev, bias, mask=None):
    """The premise of every constant-head test: want_logits returns exactly the bias at legal actions and exactly
    float32(-1e8) at illegal ones.  logits_dev: float32 numpy [N, A] read back from the device."""
    got = np.ascontiguousarray(logits_dev, dtype=np.float32).view(np.uint32)
    want = np.broadcast_to(np.asarray(bias, dtype=np.float32), logits_dev.shape).copy().view(np.uint32)
    if mask is not None:
        want[~np.asarray(mask).astype(bool)] = HUGE_NEG_BITS
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"constant head: logit bits {got[tuple(bad[0])]:#x} vs {want[tuple(bad[0])]:#x} at {bad[0].tolist()}"


def torch_reference(w, obs, mask):
    """obs [N, D] cpu, mask [N, A] bool cpu or None -> masked logits, log-softmax, value, in the dtype of w."""
    import torch
    import torch.nn.functional as F

    hp = torch.tanh(F.linear(torch.tanh(F.linear(obs, w["mlp_extractor.policy_net.0.weight"],
                                                 w["mlp_extractor.policy_net.0.bias"])),
                             w["mlp_extractor.policy_net.2.weight"], w["mlp_extractor.policy_net.2.bias"]))
    hv = torch.tanh(F.linear(torch.tanh(F.linear(obs, w["mlp_extractor.value_net.0.weight"],
                                                 w["mlp_extractor.value_net.0.bias"])),
                             w["mlp_extractor.value_net.2.weight"], w["mlp_extractor.value_net.2.bias"]))
    logits = F.linear(hp, w["action_net.weight"], w["action_net.bias"])
    if mask is not None:
        logits = torch.where(mask, logits, torch.tensor(-1e8, dtype=logits.dtype))
    value = F.linear(hv, w["value_net.weight"], w["value_net.bias"]).squeeze(1)
    return logits, torch.log_softmax(logits, dim=1), value


# ---- the sampler on a uniform policy, bit for bit ---------------------------------------------------------------------
def uniform_sample_f32(words, mask, A, NR=None):
    """The action sample_tile<NR> picks when every legal logit is 0 (bias 0 on the constant head), restated in IEEE
    float32: every legal register has mass exp2(0) = 1, running sums are small integers, and the inverse cdf is
      target = f32(word >> 8) * 2^-24 * total;  half 1 walks target - S.lo;  tl = min(tl, S_half * (1 - 2^-23));
      the first register of the half whose running count exceeds tl, else the last;  half 1 is taken iff
      !(target < S.lo) and S.hi > 0.
    words: uint [N]; mask: [N, A] (None = all legal), at least one legal action per row -> int32 [N]."""
    f32 = np.float32
    NR = kernel_regs(A) if NR is None else NR
    w = np.asarray(words, dtype=np.uint64) & np.uint64(0xFFFFFFFF)
    n = w.shape[0]
    mask = np.ones((n, A), dtype=bool) if mask is None else np.asarray(mask).astype(bool)
    assert mask.shape == (n, A) and mask.any(axis=1).all()
    legal = np.zeros((2, n, NR), dtype=bool)  # [half, row, register]; phantoms (row_of >= A) hold no mass
    for h in (0, 1):
        for r in range(NR):
            if row_of(r, h) < A:
                legal[h, :, r] = mask[:, row_of(r, h)]
    c = np.cumsum(legal.astype(f32), axis=2, dtype=f32)
    S = c[:, :, NR - 1]
    total = (S[0] + S[1]).astype(f32)
    target = ((w >> np.uint64(8)).astype(f32) * f32(2.0 ** -24)) * total
    take_hi = ~(target < S[0]) & (S[1] > f32(0))
    idx = np.empty((2, n), dtype=np.int64)
    for h in (0, 1):
        tl = (target - S[0]).astype(f32) if h else target
        tl = np.minimum(tl, (S[h] * f32(0.99999988079071044921875)).astype(f32))
        gt = c[h, :, :NR - 1] > tl[:, None]
        idx[h] = np.where(gt.any(axis=1), np.argmax(gt, axis=1), NR - 1) if NR > 1 else NR - 1
    pick = np.where(take_hi, idx[1], idx[0])
    return ((pick & 3) + 8 * (pick >> 2) + 4 * take_hi.astype(np.int64)).astype(np.int32)


def first_legal_register(mask_row, A):
    return next(a for a in register_order(A) if mask_row[a])


def last_legal_register(mask_row, A):
    return next(a for a in reversed(register_order(A)) if mask_row[a])


# ---- the forward checker ---------------------------------------------------------------------------------------------
def forward_inputs(obs_dim, n_actions, n, seed=5, edges=True):
    """edges=False: the n random rows alone.  Otherwise n random rows in [-1, 1] under 60 % masks with action 0 legal, then six edge rows (all -1, all 0, all +1, each
    once with only action 0 legal and once all-legal) -> obs [n + 6, D], mask [n + 6, A], `single` (rows with one legal
    action)."""
    import torch

    g = torch.Generator().manual_seed(seed)
    # observations lie in [-1, 1]: the obs clip, and four sort-obs slots are purity - 0.9 (env_super.py:339-359)
    obs = torch.rand((n, obs_dim), generator=g) * 2.0 - 1.0
    mask = torch.rand((n, n_actions), generator=g) < 0.6
    mask[:, 0] = True  # action 0 is always valid in the reference's masks
    if not edges:
        return obs, mask, torch.zeros(n, dtype=torch.bool)
    edge = torch.tensor([-1.0, 0.0, 1.0]).repeat_interleave(2).unsqueeze(1).expand(6, obs_dim)
    only0 = torch.zeros((6, n_actions), dtype=torch.bool)
    only0[:, 0] = True
    only0[1::2] = True
    obs, mask = torch.cat([obs, edge]), torch.cat([mask, only0])
    single = torch.zeros(n + 6, dtype=torch.bool)
    single[n::2] = True
    return obs, mask, single


def check_forward(pol, w_ref, obs, mask, single, logit_tol, seed=77, t=3, index_offset=0, report=None):
    """mse_policy_forward (through MlpPolicy `pol`) against torch's evaluation of `w_ref` (float32 or float64 tensors)
    on the same rows: logits, value, log-probability of the sampled action, legality, the inverse cdf in register
    order recomputed in float64 from the device's own logits (a draw within 1e-5 of a boundary may fall on either
    side), and the argmax on rows whose top-2 margin exceeds 1e-4 - once with the mask and once without.
    report: a dict that receives the largest logit / value errors seen."""
    import torch

    n, A = obs.shape[0], pol.n_actions
    rt = w_ref["action_net.bias"].dtype
    order = register_order(A)
    assert sorted(order) == list(range(A))
    u = ps.uniform24(ps.word(seed, index_offset + np.arange(n), t))
    for mk in (mask, None):
        ref_logits, ref_logsm, ref_value = torch_reference(w_ref, obs.to(rt), mk)
        dm = None if mk is None else mk.cuda()
        out = pol.forward(obs.cuda(), dm, seed=seed, t=t, want_logits=True, index_offset=index_offset)
        logits = out["logits"].cpu()
        err_l = float((logits.to(rt) - ref_logits).abs().max())
        err_v = float((out["value"].cpu().to(rt) - ref_value).abs().max())
        if report is not None:
            report["logits"] = max(report.get("logits", 0.0), err_l)
            report["value"] = max(report.get("value", 0.0), err_v)
        assert torch.allclose(logits.to(rt), ref_logits, atol=logit_tol, rtol=1e-6), err_l
        assert torch.allclose(out["value"].cpu().to(rt), ref_value, atol=LOGIT_TOL, rtol=1e-6), err_v
        act = out["action"].cpu().long()
        assert bool(((act >= 0) & (act < A)).all())
        if mk is not None:
            assert bool(mk.gather(1, act.unsqueeze(1)).all()), "a masked action was sampled"
        # log-probability of the sampled action
        assert torch.allclose(out["logp"].cpu().to(rt), ref_logsm.gather(1, act.unsqueeze(1)).squeeze(1), atol=LOGP_TOL)
        if mk is not None and bool(single.any()):  # a single valid action: taken with certainty
            assert bool((act[single] == 0).all()) and float(out["logp"].cpu()[single].abs().max()) <= LOGP_TOL
        # the sample is the inverse cdf of the engine's stream over the softmax masses in REGISTER order
        p = torch.softmax(logits.double(), dim=1).numpy()[:, order]
        cdf = np.cumsum(p, axis=1)
        k = np.minimum((cdf <= u[:, None]).sum(axis=1), A - 1)  # searchsorted(cdf[i], u[i], side="right")
        want = np.asarray(order)[k]
        near = np.abs(cdf - u[:, None]).min(axis=1)
        bad = np.flatnonzero((act.numpy() != want) & ~(near < 1e-5))
        assert bad.size == 0, (int(bad[0]), int(act[bad[0]]), int(want[bad[0]]), float(u[bad[0]]), cdf[bad[0]])
        # deterministic = argmax of the masked logits
        det = pol.forward(obs.cuda(), dm, deterministic=True, index_offset=index_offset)["action"].cpu().long()
        if A > 1:
            top2 = torch.topk(ref_logits, 2, dim=1).values
            clear = (top2[:, 0] - top2[:, 1]) > 1e-4
            assert bool((det[clear] == ref_logits.argmax(dim=1)[clear]).all())
        else:
            assert bool((det == 0).all())
