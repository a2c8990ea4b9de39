"""Plain-torch restatements the PPO learner tests are held against (not a test module): SB3's GAE loop in numpy
float32, the loss of MaskablePPO.train for one minibatch differentiated by autograd in any dtype, clip_grad_norm_ +
Adam, and the yardstick rule of the tolerances.

Tolerance rule (gradient): the yardstick is the float64 evaluation; an independent float32 evaluation of the same
graph by torch on the CPU has error e32 = max|g32 - g64| / max|g64|, and the code under test is allowed 4 x e32 (the
factor covers a different summation order over up to 2^20 rows).  Nothing is taken from the code under test.
Scalars (loss terms, statistics): one f32 scalar's error against float64 can be zero by accident, so the scalar bound
is 4 x the largest f32-yardstick error among the eight statistics plus 4 ulp of float32 at the statistic's magnitude
(the result is stored as a float32 after a division by the batch size: two roundings, doubled for the sum of terms).
"""
import numpy as np
import torch
import torch.nn.functional as F

SB3_KEYS = [
    "mlp_extractor.policy_net.0.weight", "mlp_extractor.policy_net.0.bias",
    "mlp_extractor.policy_net.2.weight", "mlp_extractor.policy_net.2.bias",
    "action_net.weight", "action_net.bias",
    "mlp_extractor.value_net.0.weight", "mlp_extractor.value_net.0.bias",
    "mlp_extractor.value_net.2.weight", "mlp_extractor.value_net.2.bias",
    "value_net.weight", "value_net.bias",
]
STAT_NAMES = ("loss", "policy_loss", "value_loss", "entropy_loss", "approx_kl", "clip_fraction", "adv_mean", "adv_std")


def shapes(D, A, H=32):
    return [(H, D), (H,), (H, H), (H,), (A, H), (A,), (H, D), (H,), (H, H), (H,), (1, H), (1,)]


def num_weights(D, A):
    return sum(int(np.prod(s)) for s in shapes(D, A))


def split(flat, D, A):
    out, at = [], 0
    for s in shapes(D, A):
        n = int(np.prod(s))
        out.append(flat[at:at + n].reshape(s))
        at += n
    return out


def random_flat(D, A, seed, saturating=False):
    """SB3-scale weights, or the saturating set of tests/test_gpu_policy.py (hidden layers 8x, action head gain 3)."""
    g = torch.Generator().manual_seed(seed)
    parts = []
    for k, s in zip(SB3_KEYS, shapes(D, A)):
        if len(s) == 1:
            parts.append((torch.randn(s, generator=g) * 0.1).float().ravel())
        else:
            if saturating:
                gain = 3.0 if k == "action_net.weight" else (1.0 if k == "value_net.weight" else 8.0 * 2.0 ** 0.5)
            else:
                gain = 0.5 * s[1] ** 0.5
            parts.append((torch.randn(s, generator=g) * gain / s[1] ** 0.5).float().ravel())
    return torch.cat(parts)


def forward(flat, D, A, obs, mask):
    """-> log-softmax of the masked logits [B, A], value [B]"""
    w1, b1, w2, b2, wa, ba, v1, c1, v2, c2, wv, bv = split(flat, D, A)
    hp = torch.tanh(F.linear(torch.tanh(F.linear(obs, w1, b1)), w2, b2))
    hv = torch.tanh(F.linear(torch.tanh(F.linear(obs, v1, c1)), v2, c2))
    logits = F.linear(hp, wa, ba)
    if mask is not None:
        logits = torch.where(mask, logits, torch.tensor(-1e8, dtype=logits.dtype))
    return torch.log_softmax(logits, dim=1), F.linear(hv, wv, bv).squeeze(1)


def make_rows(D, A, B, seed, flat, masked):
    """B rows whose first ones are the edge cases: a single legal action; ratios clipped below / above the range with
    advantages of both signs; a ratio inside the range.  -> obs f32[B, D], mask bool[B, A], mask or None (what the
    loss is given), actions i32[B], old_logp, adv, ret f32[B]."""
    g = torch.Generator().manual_seed(seed)
    obs = torch.rand((B, D), generator=g) * 2.0 - 1.0
    mask = torch.rand((B, A), generator=g) < 0.6
    mask[:, 0] = True
    if B > 0:
        mask[0] = False
        mask[0, 0] = True  # a single legal action
    mk = mask if masked else None
    with torch.no_grad():
        logsm, value = forward(flat.double(), D, A, obs.double(), mk)
    legal = mask if masked else torch.ones_like(mask)
    actions = torch.multinomial(legal.float(), 1, generator=g).squeeze(1).int()
    logp = logsm.gather(1, actions.long().unsqueeze(1)).squeeze(1)
    # old log-probabilities: the ratio exp(logp - old) spread over [0.6, 1.5], so both clip sides and the inside occur
    log_ratio = torch.log(torch.rand(B, generator=g, dtype=torch.float64) * 0.9 + 0.6)
    for i, lr in enumerate([0.0, np.log(0.5), np.log(0.5), np.log(1.6), np.log(1.6), np.log(1.05), np.log(0.95)][:B]):
        log_ratio[i] = lr
    old_logp = (logp - log_ratio).float()
    adv = torch.randn(B, generator=g) * 1.5 + 0.3
    for i, a in enumerate([0.7, 1.0, -1.0, 1.0, -1.0, 1.0, -1.0][:B]):
        adv[i] = a
    # returns at least 0.5 away from the value: with B = 1 the whole value-net gradient is proportional to the single
    # difference (value - returns), and a draw with |value - returns| = 0.18 turned the check into a comparison of two
    # float32 roundings of one scalar (header 2.5 ulp off in the value, torch's float32 0.4 ulp: 1.7e-6 against a bound
    # of 1.3e-6) - cancellation luck, not arithmetic.  Applied to every row alike.
    noise = torch.randn(B, generator=g, dtype=torch.float64) * 0.5
    ret = (value + torch.where(noise < 0, noise - 0.5, noise + 0.5)).float()
    return obs, mask, mk, actions, old_logp, adv, ret


def ppo_loss(flat, D, A, obs, mask, actions, old_logp, adv, ret, clip_range, ent_coef, vf_coef, normalize=True):
    """MaskablePPO.train for one minibatch -> (loss, stats[8]) in flat's dtype.  mask: bool [B, A] or None."""
    dt = flat.dtype
    obs, old_logp, adv, ret = obs.to(dt), old_logp.to(dt), adv.to(dt), ret.to(dt)
    mean, std = torch.zeros((), dtype=dt), torch.ones((), dtype=dt)
    if normalize and adv.numel() > 1:
        mean, std = adv.mean(), adv.std()
        adv = (adv - mean) / (std + 1e-8)
    logsm, value = forward(flat, D, A, obs, mask)
    logp = logsm.gather(1, actions.long().unsqueeze(1)).squeeze(1)
    ratio = torch.exp(logp - old_logp)
    pl1 = adv * ratio
    pl2 = adv * torch.clamp(ratio, 1 - clip_range, 1 + clip_range)
    policy_loss = -torch.min(pl1, pl2).mean()
    value_loss = F.mse_loss(ret, value)
    plogp = logsm * logsm.exp()
    if mask is not None:
        plogp = torch.where(mask, plogp, torch.zeros((), dtype=dt))
    entropy_loss = -(-plogp.sum(dim=1)).mean()
    loss = policy_loss + ent_coef * entropy_loss + vf_coef * value_loss
    with torch.no_grad():
        log_ratio = logp - old_logp
        kl = ((ratio - 1) - log_ratio).mean()
        clip_fraction = ((ratio - 1).abs() > clip_range).to(dt).mean()
    stats = torch.stack([loss.detach(), policy_loss.detach(), value_loss.detach(), entropy_loss.detach(), kl, clip_fraction,
                         mean.detach(), std.detach()])
    return loss, stats


def loss_and_grad(flat, dtype, *args, **kw):
    w = flat.detach().to(dtype).clone().requires_grad_(True)
    loss, stats = ppo_loss(w, *args, **kw)
    loss.backward()
    return w.grad.detach(), stats


def grad_bound(g64, g32):
    """(scale, allowed relative error) of the tolerance rule above"""
    scale = float(g64.abs().max())
    return scale, 4.0 * float((g32.double() - g64).abs().max()) / scale


def stats_bound(s64, s32, e32_others=0.0):
    """e32_others (B <= 2 only, where one evaluation's float32 error is a single draw of a heavy-tailed quantity): the
    largest float32 error of the statistics among evaluations of the same size on other rows - torch alone."""
    e32 = max(float((s32.double() - s64).abs().max()), e32_others)
    return 4.0 * e32 + 4.0 * float(np.finfo(np.float32).eps) * np.maximum(1.0, np.abs(s64.numpy()))


def gae_numpy(rewards, values, episode_starts, last_values, last_dones, gamma, gae_lambda):
    """stable_baselines3.common.buffers.RolloutBuffer.compute_returns_and_advantage, transcribed; float32 arrays."""
    K = rewards.shape[0]
    rewards, values = rewards.astype(np.float32), values.astype(np.float32)
    episode_starts = episode_starts.astype(np.float32)
    last_values = last_values.astype(np.float32)
    advantages = np.zeros_like(rewards)
    last_gae_lam = 0
    for step in reversed(range(K)):
        if step == K - 1:
            next_non_terminal = 1.0 - last_dones.astype(np.float32)
            next_values = last_values
        else:
            next_non_terminal = 1.0 - episode_starts[step + 1]
            next_values = values[step + 1]
        delta = rewards[step] + gamma * next_values * next_non_terminal - values[step]
        last_gae_lam = delta + gamma * gae_lambda * next_non_terminal * last_gae_lam
        advantages[step] = last_gae_lam
    returns = advantages + values
    assert advantages.dtype == np.float32 and returns.dtype == np.float32
    return advantages, returns


def adam_reference(w0, grads, lr, eps, max_grad_norm, dtype=torch.float64, start_step=0, m0=None, v0=None, states=None):
    """clip_grad_norm_ + torch.optim.Adam over the gradient sequence -> list of weights after each step, norms.
    start_step / m0 / v0: the optimiser's state before the first gradient (default: a fresh one).  states: a list that
    receives (exp_avg, exp_avg_sq) after each step."""
    w = torch.nn.Parameter(w0.detach().to(dtype).clone())
    opt = torch.optim.Adam([w], lr=lr, eps=eps)
    if start_step or m0 is not None or v0 is not None:
        opt.state[w] = {"step": torch.tensor(float(start_step)),
                        "exp_avg": torch.zeros_like(w.data) if m0 is None else m0.detach().to(dtype).clone(),
                        "exp_avg_sq": torch.zeros_like(w.data) if v0 is None else v0.detach().to(dtype).clone()}
    out, norms = [], []
    for g in grads:
        w.grad = g.detach().to(dtype).clone()
        if max_grad_norm > 0:
            norms.append(float(torch.nn.utils.clip_grad_norm_([w], max_grad_norm)))
        else:
            norms.append(float(w.grad.norm()))
        opt.step()
        out.append(w.detach().clone())
        if states is not None:
            states.append((opt.state[w]["exp_avg"].detach().clone(), opt.state[w]["exp_avg_sq"].detach().clone()))
    return out, norms
