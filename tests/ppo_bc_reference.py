"""Plain-torch restatement of PPO with an auxiliary imitation term (mse_ppo_bc_loss_grad), its twelve statistics and,
through autograd in any dtype, its gradient; and the rows its tests use (not a test module).  tests/ppo_reference.py (R),
tests/ppo_vclip_reference.py (V) and tests/bc_reference.py (B) are imported, not edited.

    loss   = policy_loss + ent_coef * entropy_loss + vf_coef * value_loss + bc_coef * bc_loss
             (the first three terms are R.ppo_loss, or V.ppo_loss_vclip with old_values)
    usable = the label (clamped into [0, A)) is legal under the mask
    bc_loss = mean(usable ? -log_softmax(masked logits)[label] : 0)
    stats  = loss, R's seven others, bc_loss, hits / B, unusable / B, 0
    hit    = usable and argmax(masked logits) == label, ties to the lowest index

Tolerances are R.grad_bound / R.stats_bound: 4 x torch's own float32 error against float64, computed each run.  Hits and
unusable rows are counts and are compared exactly, so no row may leave the argmax to rounding: make_kick_rows draws more
rows than it needs with R.make_rows (or V.make_vclip_rows) and keeps the first B whose two largest LEGAL logits are at
least B.ARGMAX_MARGIN apart in float64 (bc_reference.py says why 1e-3 is fifty times float32's error); assert_margins
asserts that it held.  A dropped row is replaced by a later one, so R's fixed edge rows (the clipped ratios of both signs)
stay in front whenever their argmax is clear, and every tensor of a row stays consistent with its observation.
Labels: about 60 % are the float64 argmax (hits), the rest another legal action; masked, the first two rows after row 0
that have an illegal action are labelled with an ILLEGAL one (unusable rows); row 0 has a single legal action.
"""
import numpy as np
import torch

from tests import bc_reference as B
from tests import ppo_reference as R
from tests import ppo_vclip_reference as V

STAT_NAMES = R.STAT_NAMES + ("bc_loss", "bc_accuracy", "bc_unusable", "reserved")
HP = dict(clip_range=0.2, ent_coef=0.05, vf_coef=0.5)
C_VF = 0.2
BC_COEFS = (0.0, 0.5, 4.0)


def make_kick_rows(D, A, n, seed, flat, masked, with_old=False):
    """-> dict of CPU tensors: obs f32[n, D], mask bool[n, A], mk (mask or None: what the loss is given), actions i32[n],
    old_logp, adv, ret f32[n], old (f32[n] or None), labels i32[n]"""
    draw = 2 * n + 32
    if with_old:
        obs, mask, mk, actions, old_logp, adv, ret, old = V.make_vclip_rows(D, A, draw, seed, flat, masked, C_VF)
    else:
        obs, mask, mk, actions, old_logp, adv, ret = R.make_rows(D, A, draw, seed, flat, masked)
        old = None
    keep = torch.nonzero(B.argmax_gap(flat, D, A, obs, mk)[1] >= B.ARGMAX_MARGIN).squeeze(1)[:n]
    assert keep.numel() == n, (D, A, n, seed, keep.numel())
    obs, mask, actions, old_logp, adv, ret = (t[keep].contiguous() for t in (obs, mask, actions, old_logp, adv, ret))
    old = None if old is None else old[keep].contiguous()
    mk = mask if masked else None
    g = torch.Generator().manual_seed(seed + 104729)
    best, _ = B.argmax_gap(flat, D, A, obs, mk)
    legal = mask if masked else torch.ones_like(mask)
    other = torch.multinomial(legal.float(), 1, generator=g).squeeze(1)
    labels = torch.where(torch.rand(n, generator=g) < 0.6, best, other)
    if masked:
        for i in [int(r) for r in torch.nonzero(~mask[1:].all(dim=1))[:2, 0] + 1]:
            labels[i] = int(torch.nonzero(~mask[i])[0])  # an illegal label
    return dict(obs=obs, mask=mask, mk=mk, actions=actions, old_logp=old_logp, adv=adv, ret=ret, old=old, labels=labels.int())


def assert_margins(flat, D, A, rows):
    B.assert_margins(flat, D, A, rows["obs"], rows["mk"])
    if rows["old"] is not None:
        V.assert_margins(flat, D, A, rows["obs"], rows["mk"], rows["ret"], rows["old"], C_VF, fixed_rows=False)


def take(rows, idx):
    """the rows `idx` (a LongTensor) of a row dict"""
    return {k: (None if v is None else v[idx].contiguous()) for k, v in rows.items()}


def ppo_bc_loss(flat, D, A, rows, bc_coef, hp=HP, normalize=True):
    """-> (loss, stats[12]) in flat's dtype"""
    dt = flat.dtype
    base = (D, A, rows["obs"], rows["mk"], rows["actions"], rows["old_logp"], rows["adv"], rows["ret"])
    if rows["old"] is None:
        ppo, s8 = R.ppo_loss(flat, *base, hp["clip_range"], hp["ent_coef"], hp["vf_coef"], normalize)
    else:
        ppo, s8 = V.ppo_loss_vclip(flat, *base, rows["old"], hp["clip_range"], hp["ent_coef"], hp["vf_coef"], C_VF, normalize)
    mask, n = rows["mk"], rows["obs"].shape[0]
    lab = rows["labels"].long().clamp(0, A - 1)
    logsm = R.forward(flat, D, A, rows["obs"].to(dt), mask)[0]
    usable = torch.ones(n, dtype=torch.bool) if mask is None else mask.gather(1, lab.unsqueeze(1)).squeeze(1)
    ce = torch.where(usable, -logsm.gather(1, lab.unsqueeze(1)).squeeze(1), torch.zeros((), dtype=dt))
    bc = ce.mean()
    loss = ppo + bc_coef * bc
    with torch.no_grad():
        ll = logsm if mask is None else torch.where(mask, logsm, torch.tensor(float("-inf"), dtype=dt))
        idx = torch.arange(A).expand_as(ll)
        best = torch.where(ll == ll.max(dim=1, keepdim=True).values, idx, torch.full_like(idx, A)).min(dim=1).values
        accuracy = (usable & (best == lab)).to(dt).mean()
        unusable = (~usable).to(dt).mean()
    stats = torch.cat([loss.detach().reshape(1), s8[1:], torch.stack([bc.detach(), accuracy, unusable, torch.zeros((), dtype=dt)])])
    return loss, stats


def loss_and_grad(flat, dtype, *args, **kw):
    w = flat.detach().to(dtype).clone().requires_grad_(True)
    loss, stats = ppo_bc_loss(w, *args, **kw)
    loss.backward()
    return w.grad.detach(), stats


def reference(flat, D, A, rows, bc_coef, hp=HP, normalize=True, others=None):
    """-> (g64, s64, s32, scale, allowed, e32_others): float64 autograd and R's bound from torch's own float32 error.
    others (batches of one or two rows): row dicts of the same size whose float32 errors widen the yardstick, as
    tests/ppo_checks.py does for such batches (one evaluation's float32 error is a single draw of a heavy-tailed
    quantity) - torch alone."""
    g64, s64 = loss_and_grad(flat, torch.float64, D, A, rows, bc_coef, hp, normalize)
    g32, s32 = loss_and_grad(flat, torch.float32, D, A, rows, bc_coef, hp, normalize)
    scale, allowed = R.grad_bound(g64, g32)
    e32_others = 0.0
    for o in others or ():
        o64, t64 = loss_and_grad(flat, torch.float64, D, A, o, bc_coef, hp, normalize)
        o32, t32 = loss_and_grad(flat, torch.float32, D, A, o, bc_coef, hp, normalize)
        if float(o64.abs().max()) > 0.0:  # (a clipped ratio, a clipped value and one legal action: a row that teaches nothing)
            allowed = max(allowed, R.grad_bound(o64, o32)[1])
        e32_others = max(e32_others, float((t32.double() - t64).abs().max()))
    return g64, s64, s32, scale, allowed, e32_others


def check(label, g, s, ref):
    """g f32[W], s [12] (CPU) from the code under test against `reference`'s tuple; the counts exactly"""
    g64, s64, s32, scale, allowed, e32_others = ref
    assert bool(torch.isfinite(g).all()) and bool(torch.isfinite(s).all()), label
    err = float((g.double() - g64).abs().max()) / scale
    serr = np.abs(s.double().numpy() - s64.numpy())
    print(f"{label}: grad err {err:.3e}, f32 yardstick {allowed / 4:.3e} (allowed {allowed:.3e}); stats err {serr.max():.3e}; "
          f"loss {float(s64[0]):.6f} bc_loss {float(s64[8]):.4f} accuracy {float(s64[9]):.4f} unusable {float(s64[10]):.4f}")
    assert err <= allowed, (label, err, allowed)
    assert np.all(serr <= R.stats_bound(s64, s32, e32_others)), (label, s, s64)
    assert float(s[9]) == float(s64[9].float()) and float(s[10]) == float(s64[10].float()), (label, s[9:11], s64[9:11])
    assert float(s[11]) == 0.0, label
