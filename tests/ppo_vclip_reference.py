"""Plain-torch restatement of the PPO loss with SB3's clip_range_vf, and the rows the value-clipping tests use (not a test
module).  tests/ppo_reference.py (R) is imported, not edited: the loss below is R.ppo_loss with
value = old + clamp(value - old, -c, c), differentiated by autograd in any dtype as R.loss_and_grad does, and the
tolerances are R.grad_bound / R.stats_bound (4 x torch's own float32 error against float64, computed each run).

Rows.  The clamp's indicator is discontinuous: a row whose |value - old| sat at c would be clipped in one precision and
not in the other, and prove nothing.  make_vclip_rows therefore builds old_values from the FLOAT64 value of R.forward
with a margin:  | |value64 - old| - c | >= margin(c)  and  |vp64 - returns| >= 0.5  for every row (vp64 the clipped
float64 prediction; 0.5 is R.make_rows' own margin, for its reason).  margin(c) = min(0.05, c / 2): 0.05 wherever a row
inside the range can have it (c = 0.2), and half the range at c = 0.05, where |d| <= c - 0.05 = 0 would leave no row
inside at all; float32's error in a value is below 1e-5, two thousand times smaller than either.  Rows 0 .. 5 are fixed:
inside the range, clipped above, clipped below, each with returns above and below the prediction; of the others about
half are clipped.  assert_margins checks both conditions on the float64 reference; the tests call it before they use rows.
"""
import torch
import torch.nn.functional as F

from tests import ppo_reference as R

RET_MARGIN = 0.5

# what tests/test_gpu_ppo_vclip.py draws, so that tests/test_ppo_vclip_cpu.py can check the margins of every one of them
# without a device: (D, A, seed of R.random_flat, rows, seed of make_vclip_rows), all masked, c = GPU_C
GPU_C = 0.2
EDGE_SHAPES = [(29, 22), (32, 32)]
EDGE_BATCHES = [1, 2, 63, 64, 65, 129, 193]
EDGE_ROWS = 193 + 128
CAP_FLAT_SEED, CAP_ROW_SEED = 43, 5
SMALL_FLAT_SEED, SMALL_ROW_SEED = 53, 9  # the 300-row (29, 22) set of the tests that are not about shapes


def gpu_row_sets(group_cap=512):
    from tests.ppo_checks import DIM_MATRIX

    sets = [(D, A, D * 100 + A, 300, 11) for D, A in DIM_MATRIX]
    sets += [(D, A, 41, EDGE_ROWS, B) for D, A in EDGE_SHAPES for B in EDGE_BATCHES]
    sets += [(29, 22, CAP_FLAT_SEED, 128 * group_cap + 65, CAP_ROW_SEED), (29, 22, SMALL_FLAT_SEED, 300, SMALL_ROW_SEED)]
    return sets


def margin(c):
    return min(0.05, c / 2.0)


def make_vclip_rows(D, A, B, seed, flat, masked, c):
    """R.make_rows(D, A, B, seed, flat, masked) with `ret` replaced and old_values added
    -> obs, mask, mk, actions, old_logp, adv, ret, old_values (f32[B])."""
    obs, mask, mk, actions, old_logp, adv, _ = R.make_rows(D, A, B, seed, flat, masked)
    g = torch.Generator().manual_seed(seed + 7919)
    with torch.no_grad():
        value = R.forward(flat.double(), D, A, obs.double(), mk)[1]
    m, slack = margin(c), 1e-3
    inside = (torch.rand(B, generator=g, dtype=torch.float64) * 2.0 - 1.0) * (c - m - slack)
    clipped = c + m + slack + torch.rand(B, generator=g, dtype=torch.float64) * 0.3
    clipped = torch.where(torch.rand(B, generator=g) < 0.5, clipped, -clipped)
    d = torch.where(torch.rand(B, generator=g) < 0.5, inside, clipped)
    side = torch.where(torch.rand(B, generator=g) < 0.5, 1.0, -1.0).double()
    big = c + m + 0.1
    fixed = [(0.4 * (c - m), 1.0), (-0.4 * (c - m), -1.0), (big, 1.0), (big, -1.0), (-big, 1.0), (-big, -1.0)]
    for i, (di, si) in enumerate(fixed[:B]):
        d[i], side[i] = di, si
    old = (value - d).float()  # value - old = d up to old's rounding
    vp = old.double() + torch.clamp(value - old.double(), -c, c)
    noise = torch.rand(B, generator=g, dtype=torch.float64)
    ret = (vp + side * (RET_MARGIN + slack + noise)).float()
    return obs, mask, mk, actions, old_logp, adv, ret, old


def assert_margins(flat, D, A, obs, mk, ret, old, c, fixed_rows=True):
    """both conditions of the module docstring on the float64 reference; -> the number of clipped rows"""
    with torch.no_grad():
        value = R.forward(flat.double(), D, A, obs.double(), mk)[1]
    d = value - old.double()
    assert bool(((d.abs() - c).abs() >= margin(c)).all()), float(((d.abs() - c).abs()).min())
    vp = old.double() + torch.clamp(d, -c, c)
    assert bool(((vp - ret.double()).abs() >= RET_MARGIN).all()), float((vp - ret.double()).abs().min())
    B = obs.shape[0]
    if fixed_rows and B >= 6:
        assert (d[:6].abs() > c).tolist() == [False, False, True, True, True, True]
        assert (d[:6] > 0).tolist() == [True, False, True, True, False, False]
        assert (ret[:6].double() > vp[:6]).tolist() == [True, False, True, False, True, False]
    return int((d.abs() > c).sum())


def ppo_loss_vclip(flat, D, A, obs, mask, actions, old_logp, adv, ret, old_values, clip_range, ent_coef, vf_coef, clip_range_vf,
                   normalize=True):
    """MaskablePPO.train for one minibatch with clip_range_vf -> (loss, stats[8]) in flat's dtype: R.ppo_loss, its value
    replaced by old_values + clamp(value - old_values, -clip_range_vf, clip_range_vf)."""
    dt = flat.dtype
    obs, old_logp, adv, ret, old_values = obs.to(dt), old_logp.to(dt), adv.to(dt), ret.to(dt), old_values.to(dt)
    mean, std = torch.zeros((), dtype=dt), torch.ones((), dtype=dt)
    if normalize and adv.numel() > 1:
        mean, std = adv.mean(), adv.std()
        adv = (adv - mean) / (std + 1e-8)
    logsm, value = R.forward(flat, D, A, obs, mask)
    value = old_values + torch.clamp(value - old_values, -clip_range_vf, clip_range_vf)
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
    loss, stats = ppo_loss_vclip(w, *args, **kw)
    loss.backward()
    return w.grad.detach(), stats
