"""Plain-torch restatement of the behaviour-cloning loss (mse_bc_loss_grad), its statistics and, through autograd in any
dtype, its gradient; and the rows the behaviour-cloning tests use (not a test module).  tests/ppo_reference.py (R) is
imported, not edited: the networks are R.forward, the tolerances R.grad_bound / R.stats_bound (4 x torch's own float32
error against float64, computed each run).

    usable   = the label (clamped into [0, A)) is legal under the mask
    bc_loss  = mean(usable ? -log_softmax(masked logits)[label] : 0)
    loss     = bc_loss + ent_coef * entropy_loss + vf_coef * value_loss        (value_loss = 0 without returns)
    stats    = loss, bc_loss, value_loss, entropy_loss, hits / B, unusable / B, 0, 1
    hit      = usable and argmax(masked logits) == label, ties to the lowest index

Rows.  Accuracy is a count and is compared exactly, so no row may leave the argmax to rounding: make_bc_rows resamples
every row whose two largest LEGAL logits are closer than ARGMAX_MARGIN in float64, and assert_margins asserts that the
margin held.  ARGMAX_MARGIN = 1e-3: a logit is a 32-term dot product of numbers of order 1 at most (|tanh| <= 1, head
weights of order 1 even in the saturating set), so its float32 error is below 32 * 2^-24 * 10 = 2e-5 however the sum is
ordered - fifty times less.  Exact ties are tested separately, with the expected winner written down.
Row 0 (masked) has a single legal action.  The first two rows after it that have an illegal action (masked) demonstrate
an ILLEGAL one: unusable rows.  About 60 % of the other labels are the float64 argmax (hits), the rest another legal action.
"""
import torch

from tests import ppo_reference as R

ARGMAX_MARGIN = 1e-3
STAT_NAMES = ("loss", "bc_loss", "value_loss", "entropy_loss", "accuracy", "unusable", "_", "_")
HP = dict(ent_coef=0.05, vf_coef=0.5)


def legal_logits(flat, D, A, obs, mk):
    """float64 log-softmax of the masked logits with the illegal ones at -inf (differences are those of the logits)"""
    with torch.no_grad():
        logsm = R.forward(flat.double(), D, A, obs.double(), mk)[0]
    return logsm if mk is None else torch.where(mk, logsm, torch.tensor(float("-inf"), dtype=torch.float64))


def argmax_gap(flat, D, A, obs, mk):
    """-> (argmax with ties to the lowest index, gap between the two largest legal logits; inf with one legal action)"""
    ll = legal_logits(flat, D, A, obs, mk)
    top = ll.max(dim=1, keepdim=True).values
    idx = torch.arange(A).expand_as(ll)
    best = torch.where(ll == top, idx, torch.full_like(idx, A)).min(dim=1).values
    if A == 1:
        return best, torch.full((ll.shape[0],), float("inf"), dtype=torch.float64)
    two = ll.topk(2, dim=1).values
    return best, two[:, 0] - two[:, 1]


def assert_margins(flat, D, A, obs, mk, margin=ARGMAX_MARGIN):
    gap = argmax_gap(flat, D, A, obs, mk)[1]
    assert bool((gap >= margin).all()), float(gap.min())


def make_bc_rows(D, A, B, seed, flat, masked, margin=ARGMAX_MARGIN, edit_mask=None):
    """-> obs f32[B, D], mask bool[B, A], mk (mask or None: what the loss is given), labels i32[B], ret f32[B].
    edit_mask(mask): changes the mask in place before the rows are resampled, so the margin holds under the edited mask."""
    g = torch.Generator().manual_seed(seed)
    obs = torch.rand((B, D), generator=g) * 2.0 - 1.0
    mask = torch.rand((B, A), generator=g) < 0.6
    mask[:, 0] = True
    mask[0] = False
    mask[0, 0] = True  # a single legal action
    if edit_mask is not None:
        edit_mask(mask)
    mk = mask if masked else None
    for _ in range(200):  # resample the rows whose argmax float32 might decide otherwise
        near = argmax_gap(flat, D, A, obs, mk)[1] < margin
        if not bool(near.any()):
            break
        obs[near] = torch.rand((int(near.sum()), D), generator=g) * 2.0 - 1.0
    assert_margins(flat, D, A, obs, mk, margin)
    best, _ = argmax_gap(flat, D, A, obs, mk)
    legal = mask if masked else torch.ones_like(mask)
    other = torch.multinomial(legal.float(), 1, generator=g).squeeze(1)
    labels = torch.where(torch.rand(B, generator=g) < 0.6, best, other)
    if masked:
        for i in [int(r) for r in torch.nonzero(~mask[1:].all(dim=1))[:2, 0] + 1]:  # the first two such rows after row 0
            labels[i] = int(torch.nonzero(~mask[i])[0])  # an illegal demonstration
    with torch.no_grad():
        value = R.forward(flat.double(), D, A, obs.double(), mk)[1]
    noise = torch.randn(B, generator=g, dtype=torch.float64) * 0.5
    ret = (value + torch.where(noise < 0, noise - 0.5, noise + 0.5)).float()  # R.make_rows' margin, for its reason
    return obs, mask, mk, labels.int(), ret


def bc_loss(flat, D, A, obs, mask, labels, ret, ent_coef, vf_coef):
    """-> (loss, stats[8]) in flat's dtype.  mask: bool [B, A] or None; ret: [B] or None (actor only)."""
    dt = flat.dtype
    obs = obs.to(dt)
    B = obs.shape[0]
    lab = labels.long().clamp(0, A - 1)
    logsm, value = R.forward(flat, D, A, obs, mask)
    usable = torch.ones(B, dtype=torch.bool) if mask is None else mask.gather(1, lab.unsqueeze(1)).squeeze(1)
    ce = torch.where(usable, -logsm.gather(1, lab.unsqueeze(1)).squeeze(1), torch.zeros((), dtype=dt))
    bc = ce.mean()
    value_loss = torch.zeros((), dtype=dt) if ret is None else ((ret.to(dt) - value) ** 2).mean()
    plogp = logsm * logsm.exp()
    if mask is not None:
        plogp = torch.where(mask, plogp, torch.zeros((), dtype=dt))
    entropy_loss = -(-plogp.sum(dim=1)).mean()
    loss = bc + ent_coef * entropy_loss + vf_coef * value_loss
    with torch.no_grad():
        ll = logsm if mask is None else torch.where(mask, logsm, torch.tensor(float("-inf"), dtype=dt))
        idx = torch.arange(A).expand_as(ll)
        best = torch.where(ll == ll.max(dim=1, keepdim=True).values, idx, torch.full_like(idx, A)).min(dim=1).values
        accuracy = (usable & (best == lab)).to(dt).mean()
        unusable = (~usable).to(dt).mean()
    stats = torch.stack([loss.detach(), bc.detach(), value_loss.detach(), entropy_loss.detach(), accuracy, unusable,
                         torch.zeros((), dtype=dt), torch.ones((), dtype=dt)])
    return loss, stats


def loss_and_grad(flat, dtype, *args):
    w = flat.detach().to(dtype).clone().requires_grad_(True)
    loss, stats = bc_loss(w, *args)
    loss.backward()
    return w.grad.detach(), stats


def critic_slice(D, A):
    """the flat indices of the critic's weights (the last six blocks of the flat order)"""
    sizes = [int(torch.tensor(s).prod()) for s in R.shapes(D, A)]
    return slice(sum(sizes[:6]), sum(sizes))


def reference(flat, D, A, obs, mk, labels, ret, hp=HP, others=None):
    """-> (g64, s64, s32, scale, allowed, e32_others): float64 autograd and R's bound from torch's own float32 error.
    others (B <= 2): row sets (obs, mk, labels, ret) of the same size whose float32 errors widen the yardstick, as
    tests/ppo_checks.py does for such batches (one evaluation's float32 error is a single draw of a heavy-tailed
    quantity) - torch alone."""
    args = (D, A, obs, mk, labels, ret, hp["ent_coef"], hp["vf_coef"])
    g64, s64 = loss_and_grad(flat, torch.float64, *args)
    g32, s32 = loss_and_grad(flat, torch.float32, *args)
    scale = float(g64.abs().max())
    e32_others, allowed = 0.0, 0.0
    if scale > 0.0:
        allowed = R.grad_bound(g64, g32)[1]
    for o in others or ():
        a1 = (D, A, *o, hp["ent_coef"], hp["vf_coef"])
        (o64, t64), (o32, t32) = loss_and_grad(flat, torch.float64, *a1), loss_and_grad(flat, torch.float32, *a1)
        if float(o64.abs().max()) > 0.0:
            allowed = max(allowed, R.grad_bound(o64, o32)[1])
        e32_others = max(e32_others, float((t32.double() - t64).abs().max()))
    return g64, s64, s32, scale, allowed, e32_others


def check(label, g, s, flat, D, A, obs, mk, labels, ret, hp=HP, others=None, ref=None):
    """g f32[W], s [8] (CPU) from the code under test against `reference` (ref: one computed before and shared).  The two
    counts are compared exactly.  -> (g64, s64)"""
    import numpy as np

    g64, s64, s32, scale, allowed, e32_others = ref if ref is not None else reference(flat, D, A, obs, mk, labels, ret, hp, others)
    assert bool(torch.isfinite(g).all()) and bool(torch.isfinite(s).all()), label
    if scale == 0.0:  # one action and no returns: nothing to learn, and the code must say exactly that
        err = float(g.abs().max())
        print(f"{label}: zero gradient expected, largest entry {err:.3e}")
        assert err == 0.0, label
    else:
        err = float((g.double() - g64).abs().max()) / scale
        print(f"{label}: grad err {err:.3e}, f32 yardstick {allowed / 4:.3e} (allowed {allowed:.3e}); loss {float(s64[0]):.6f} "
              f"accuracy {float(s64[4]):.4f} unusable {float(s64[5]):.4f}")
        assert err <= allowed, (label, err, allowed)
    serr = np.abs(s.double().numpy() - s64.numpy())
    assert np.all(serr <= R.stats_bound(s64, s32, e32_others)), (label, s, s64)
    assert float(s[4]) == float(s64[4].float()) and float(s[5]) == float(s64[5].float()), (label, s[4:6], s64[4:6])
    assert float(s[6]) == 0.0 and float(s[7]) == 1.0, label
    if ret is None:
        assert bool((g[critic_slice(D, A)] == 0).all()) and float(s[2]) == 0.0, label
    return g64, s64
