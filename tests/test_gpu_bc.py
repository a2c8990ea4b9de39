"""GPU: behaviour cloning on the device - mse_bc_loss_grad (the BC instantiations of k_ppo_grad and k_ppo_grad_matrix),
DemonstrationCollector and ImitationLearner.

The gradient and the statistics are held against the float64 autograd of tests/bc_reference.py under the tolerance rule
of tests/ppo_reference.py (4 x torch's own float32 error, computed each run); accuracy and the unusable fraction are
counts and must match exactly, on rows whose argmax keeps a margin float32 cannot cross (asserted on the float64
reference).  One reference serves both arithmetics of a case."""
import functools

import numpy as np
import pytest

from tests import bc_reference as B
from tests import ppo_reference as R
from tests.ppo_checks import DIM_MATRIX, ROWS_PER_GROUP, group_cap, make_policy, same_bits

pytestmark = pytest.mark.gpu

MONO = (29, 22)
FORMS = ["fma", "matrix"]
BATCHES = [1, 63, 64, 65, 128, 129, 300]  # the tile and group edges
N_ROWS = 300 + 64  # the last 64 rows widen the yardstick of the one-row batch (tests/ppo_checks.py batch_edges)


def bc_learner(D, A, flat_seed, arithmetic, **kw):
    import marl_sortingenv_amd as M

    pol, flat = make_policy(D, A, flat_seed, precision="f32")
    return M.ImitationLearner(pol, arithmetic=arithmetic, **dict(B.HP, **kw)), flat


def device_rows(obs, mk, labels, ret):
    import torch

    d = {"observations": obs.contiguous().cuda(), "actions": labels.int().contiguous().cuda()}
    if mk is not None:
        d["action_masks"] = mk.to(dtype=torch.uint8).contiguous().cuda()
    if ret is not None:
        d["returns"] = ret.contiguous().cuda()
    return d


def run_kernel(learner, flat, data, rows_cpu, batch, grad_out=None, stats_out=None):
    """one loss_grad, twice: equal inputs must give equal bits.  -> (gradient, statistics) on the CPU"""
    import torch

    stats = torch.zeros(8, device="cuda") if stats_out is None else stats_out
    rows_dev = None if rows_cpu is None else rows_cpu.cuda()
    w_dev = flat.cuda()
    g = learner.loss_grad(data, rows_dev, batch, stats, weights=w_dev, grad_out=grad_out).clone()
    stats = stats.clone()
    stats2 = torch.full((8,), float("nan"), device="cuda")
    g2 = learner.loss_grad(data, rows_dev, batch, stats2, weights=w_dev, grad_out=torch.full_like(g, float("nan")))
    torch.cuda.synchronize()
    assert same_bits(g, g2) and same_bits(stats, stats2), "two calls with the same inputs must agree bit for bit"
    return g.cpu(), stats.cpu()


def both_forms(D, A, flat_seed, cpu, rows_cpu, batch, label, others=None, sel=None):
    """both arithmetics on one row set against ONE reference, then against each other within the same bound.
    cpu = [obs, mk, labels, ret]; sel: the rows the reference is evaluated on when they are not cpu[rows_cpu]"""
    import torch

    data = device_rows(*cpu)
    if sel is None:
        idx = torch.arange(batch) if rows_cpu is None else rows_cpu
        sel = [None if t is None else t[idx] for t in cpu]
    flat = R.random_flat(D, A, flat_seed)
    ref = B.reference(flat, D, A, *sel, others=others)
    out = {}
    for arithmetic in FORMS:
        learner, flat2 = bc_learner(D, A, flat_seed, arithmetic)
        assert torch.equal(flat, flat2)
        g, s = run_kernel(learner, flat, data, rows_cpu, batch)
        B.check(f"{arithmetic} {label}", g, s, flat, D, A, *sel, ref=ref)
        out[arithmetic] = (g, s)
    (gf, sf), (gm, sm) = out["fma"], out["matrix"]
    scale, allowed = ref[3], ref[4]
    if scale > 0.0:
        assert float((gf.double() - gm.double()).abs().max()) / scale <= allowed, label
    assert sf[4:].tolist() == sm[4:].tolist(), label  # the counts and the two constants: exactly
    return out


@functools.lru_cache(maxsize=None)
def shape_rows(D, A):
    flat = R.random_flat(D, A, D * 100 + A)
    obs, mask, mk, labels, ret = B.make_bc_rows(D, A, N_ROWS, seed=31, flat=flat, masked=True)
    B.assert_margins(flat, D, A, obs, mk)
    return [obs, mk, labels, ret]


# ---- 1. both forms against float64: every instantiation, every tile and group edge -------------------------------------------
@pytest.mark.parametrize("batch", BATCHES)
@pytest.mark.parametrize("D,A", DIM_MATRIX)
def test_every_shape_and_batch_edge(D, A, batch):
    import torch

    cpu = shape_rows(D, A)
    perm = torch.randperm(300, generator=torch.Generator().manual_seed(batch))
    for rows, name in ((None, "rows_dev=NULL"), (perm[:batch], "permuted rows_dev")):
        others = None
        if batch == 1:
            others = [[None if t is None else t[j:j + 1] for t in cpu] for j in range(300, N_ROWS)]
        both_forms(D, A, D * 100 + A, cpu, rows, batch, f"{D}->{A} B={batch} {name}", others=others)


@pytest.mark.parametrize("with_returns", [True, False])
@pytest.mark.parametrize("masked", [True, False])
@pytest.mark.parametrize("D,A", [(13, 2), (16, 11), MONO, (1, 1), (32, 32)])
def test_unmasked_and_actor_only(D, A, masked, with_returns):
    flat = R.random_flat(D, A, 61)
    obs, mask, mk, labels, ret = B.make_bc_rows(D, A, 300, seed=37, flat=flat, masked=masked)
    out = both_forms(D, A, 61, [obs, mk, labels, ret if with_returns else None], None, 300,
                     f"{D}->{A} masked={masked} returns={with_returns}")
    for g, s in out.values():
        assert s[6:].tolist() == [0.0, 1.0]
        if masked and A > 1:
            assert float(s[5]) > 0.0  # two rows demonstrate an illegal action


def test_grid_cap_second_pass():
    """128 * group_cap() + 1 rows: the first wave of workgroup 0 takes a second tile with its accumulators carried over"""
    D, A = 1, 1
    n = ROWS_PER_GROUP * group_cap() + 1
    flat = R.random_flat(D, A, 43)
    obs, mask, mk, labels, ret = B.make_bc_rows(D, A, n, seed=5, flat=flat, masked=True)
    both_forms(D, A, 43, [obs, mk, labels, ret], None, n, f"1->1 B={n} (cap {group_cap()})")


# ---- 2. indices and actions ----------------------------------------------------------------------------------------------------
def test_rows_may_repeat_and_rows_outside_are_clamped():
    import torch

    D, A = MONO
    n_rows = 100
    flat = R.random_flat(D, A, 47)
    cpu = list(B.make_bc_rows(D, A, n_rows, seed=1, flat=flat, masked=True))
    cpu = [cpu[0], cpu[2], cpu[3], cpu[4]]
    rows = torch.randint(0, n_rows, (3 * n_rows,), generator=torch.Generator().manual_seed(2))
    rows[:4] = 7
    assert rows.unique().numel() < n_rows  # some rows never occur, others repeat
    both_forms(D, A, 47, cpu, rows, rows.numel(), "mono repeated rows, batch = 3 n_rows")
    rows = torch.randperm(n_rows, generator=torch.Generator().manual_seed(4))[:80]
    rows[[0, 5, 17, 40, 79]] = torch.tensor([n_rows + 10 ** 9, -5, n_rows, n_rows + 10 ** 9, -2 ** 62])
    clamped = rows.clamp(0, n_rows - 1)
    both_forms(D, A, 47, cpu, rows, rows.numel(), "mono rows outside [0, n_rows)", sel=[t[clamped] for t in cpu])


@pytest.mark.parametrize("D,A", [MONO, (13, 2)])
def test_actions_outside_the_head_are_clamped(D, A):
    import torch

    flat = R.random_flat(D, A, 49)
    obs, mask, mk, labels, ret = B.make_bc_rows(D, A, 300, seed=5, flat=flat, masked=True)
    bad = labels.clone()
    bad[[3, 70, 150]] = -1
    bad[[4, 71, 299]] = A + 3
    bad[200] = 2 ** 31 - 1
    bad[201] = -2 ** 31
    # the reference clamps too (its labels.clamp), so the device is given the raw labels and the reference the same ones
    out = both_forms(D, A, 49, [obs, mk, bad, ret], None, 300, f"{D}->{A} actions outside [0, A)")
    same = both_forms(D, A, 49, [obs, mk, bad.clamp(0, A - 1), ret], None, 300, f"{D}->{A} the same actions clamped by hand")
    for form in FORMS:
        assert same_bits(out[form][0], same[form][0]) and same_bits(out[form][1], same[form][1])


@pytest.mark.parametrize("arithmetic", FORMS)
def test_writes_nothing_else(arithmetic):
    import torch

    D, A = MONO
    learner, flat = bc_learner(D, A, 53, arithmetic)
    obs, mask, mk, labels, ret = B.make_bc_rows(D, A, 300, seed=9, flat=flat, masked=True)
    W, band, sentinel = flat.numel(), 64, 12345.0
    gbuf = torch.full((W + 2 * band,), sentinel, device="cuda")
    sbuf = torch.full((8 + 2 * band,), sentinel, device="cuda")
    gbuf[band:band + W] = float("nan")
    sbuf[band:band + 8] = float("nan")
    g, s = run_kernel(learner, flat, device_rows(obs, mk, labels, ret), None, 300, grad_out=gbuf[band:band + W],
                      stats_out=sbuf[band:band + 8])
    B.check(f"{arithmetic} mono into banded buffers", g, s, flat, D, A, obs, mk, labels, ret)
    for buf, n in ((gbuf, W), (sbuf, 8)):
        assert bool((buf[:band] == sentinel).all()) and bool((buf[band + n:] == sentinel).all())
        assert int(torch.isfinite(buf[band:band + n]).sum()) == n


# ---- 3. the collector ----------------------------------------------------------------------------------------------------------
def _env(kind, n, max_steps, seed=7, noise=0.05):
    import marl_sortingenv_amd as M

    return M.BatchedSortingEnv(kind=kind, num_envs=n, device=0, base_seed=seed, max_steps=max_steps, noise_sorting=noise,
                               balesize=200, auto_reset=True)


def _view(env, agent):
    if agent == "own":
        return env.obs.clone(), env.mask.clone()
    if agent == "sort":
        return env.sort_agent_obs(), None
    return env.press_agent_obs(), env.mask[:, :11].clone()


K = 5


@pytest.mark.parametrize("max_steps", [3, 40])
@pytest.mark.parametrize("n", [1, 33, 257])
def test_collector_with_the_expert_stepping(n, max_steps):
    import torch

    import marl_sortingenv_amd as M

    flat_labels = {}
    for kind, agent in (("mono", "own"), ("mono", "sort"), ("mono", "press"), ("sort", "own"), ("press", "own")):
        col = M.DemonstrationCollector(_env(kind, n, max_steps), K, agent=agent, gamma=0.97)
        data = col.collect()
        buf = _env(kind, n, max_steps).rollout(K, policy="rule_based")
        torch.cuda.synchronize()
        label = f"{kind} {agent} n={n} max_steps={max_steps}"
        # the trajectory is rollout(K, policy="rule_based")'s from the same seeds, bit for bit
        assert torch.equal(data["stepped_actions"], buf["actions"]), label
        assert same_bits(data["rewards"], buf["reward"]), label
        assert torch.equal(data["episode_starts"][1:], buf["done"][:-1]) and torch.equal(data["last_dones"], buf["done"][-1]), label
        assert bool((data["episode_starts"][0] == 1).all()), label
        if max_steps == 3:
            assert bool(buf["done"].any()), "episodes end inside the window"
        if agent == "own":
            assert torch.equal(data["actions"], buf["actions"]), label
            if kind == "mono":
                flat_labels[kind] = data["actions"].clone()
        else:
            flat_labels[agent] = data["actions"].clone()
        assert data["action_masks"] is None if agent == "sort" else data["action_masks"].dtype == torch.uint8
        for key in ("observations", "action_masks", "actions", "rewards", "episode_starts", "returns"):
            assert data[key] is None or (data[key].is_contiguous() and tuple(data[key].shape[:2]) == (K, n)), (label, key)
        # row k is what the env showed before step k: a second env stepped by hand with the recorded actions
        env2 = _env(kind, n, max_steps)
        for k in range(K):
            obs, mask = _view(env2, agent)
            assert same_bits(data["observations"][k], obs), (label, k)
            if mask is not None:
                assert torch.equal(data["action_masks"][k], mask), (label, k)
            env2.step(data["stepped_actions"][k])
        # returns: the discounted reward-to-go inside the window, no bootstrap (mse_gae with zero values, lambda = 1)
        zeros = np.zeros((K, n), np.float32)
        _, er = R.gae_numpy(data["rewards"].cpu().numpy(), zeros, data["episode_starts"].cpu().numpy(), zeros[0],
                            data["last_dones"].cpu().numpy(), 0.97, 1.0)
        assert np.array_equal(data["returns"].cpu().numpy().view(np.uint32), er.view(np.uint32)), label
    # the modular labels recombine to the flat rule action
    assert torch.equal(11 * flat_labels["sort"] + flat_labels["press"], flat_labels["mono"])
    assert int(flat_labels["sort"].max()) <= 1 and int(flat_labels["press"].max()) <= 10


@pytest.mark.parametrize("deterministic", [False, True])
@pytest.mark.parametrize("agent", ["own", "sort", "press"])
def test_collector_with_an_actor_relabels_the_states_it_visits(agent, deterministic):
    import torch

    import marl_sortingenv_amd as M
    from marl_sortingenv_amd.imitation import AGENT_DIMS

    n, max_steps = 33, 3
    D, A = MONO if agent == "own" else AGENT_DIMS[agent]
    actor = M.MlpPolicy.random_init(D, A, seed=3, device=0)
    col = M.DemonstrationCollector(_env("mono", n, max_steps), K, agent=agent, actor=actor, deterministic_actor=deterministic, seed=77)
    data = col.collect()
    env2 = _env("mono", n, max_steps)
    differs = 0
    for k in range(K):
        obs, mask = _view(env2, agent)
        assert same_bits(data["observations"][k], obs)
        rule = env2.rule_actions()
        a = actor.forward(obs, mask, seed=77, t=k, deterministic=deterministic, index_offset=0)["action"]
        want_label = rule if agent == "own" else (rule // 11 if agent == "sort" else rule % 11)
        want_step = a if agent == "own" else (11 * a + rule % 11 if agent == "sort" else 11 * (rule // 11) + a)
        assert torch.equal(data["actions"][k], want_label), (agent, k)  # the label is the expert's in the visited state
        assert torch.equal(data["stepped_actions"][k], want_step), (agent, k)  # the step is the actor's
        differs += int((want_label != a).sum())
        _, rew, _, _ = env2.step(data["stepped_actions"][k])
        assert same_bits(data["rewards"][k], rew)
    if agent != "press":  # in an episode's first steps nothing can be pressed: the mask leaves the pressing agent one action
        assert differs > 0, "an untrained actor does not act like the expert"
    with pytest.raises(ValueError):
        M.DemonstrationCollector(_env("press", 4, 3), K, agent="sort")
    with pytest.raises(ValueError):
        M.DemonstrationCollector(_env("mono", 4, 3), K, agent="press", actor=M.MlpPolicy.random_init(13, 2, seed=1, device=0))


# ---- 4. the learner ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def mono_demonstrations(n=64, k=8, noise=0.05):
    import marl_sortingenv_amd as M

    return M.DemonstrationCollector(_env("mono", n, 5, seed=11, noise=noise), k).collect()


@pytest.mark.parametrize("arithmetic", FORMS)
@pytest.mark.parametrize("weight_sync", ["host", "device"])
@pytest.mark.parametrize("shuffle", ["cpu", "device"])
def test_update_is_the_hand_loop_bit_for_bit(shuffle, weight_sync, arithmetic):
    import torch

    data = mono_demonstrations()
    total, bs, epochs = 512, 100, 2  # a short last minibatch of 12 rows
    kw = dict(n_epochs=epochs, batch_size=bs, seed=5, shuffle=shuffle, weight_sync=weight_sync)
    auto, _ = bc_learner(*MONO, 71, arithmetic, **kw)
    hand, _ = bc_learner(*MONO, 71, arithmetic, **kw)
    out = auto.update(data)
    per_epoch = (total + bs - 1) // bs
    assert tuple(out["stats"].shape) == (epochs * per_epoch, 8) and auto.step == epochs * per_epoch
    assert list(out["mean"]) == ["loss", "bc_loss", "value_loss", "entropy_loss", "accuracy", "unusable", "_"]
    gen = torch.Generator().manual_seed(5)
    stats = torch.zeros((epochs * per_epoch, 8), device="cuda")
    i = 0
    for epoch in range(epochs):
        perm = (torch.randperm(total, generator=gen) if shuffle == "cpu" else hand.permutation(total, epoch)).cuda()
        if shuffle == "cpu":
            assert torch.equal(perm.cpu(), auto.last_permutations[epoch])
        for start in range(0, total, bs):
            rows = perm[start:start + bs]
            hand.loss_grad(data, rows, rows.numel(), stats[i])
            hand.adam_step()
            i += 1
    torch.cuda.synchronize()
    assert same_bits(auto.weights, hand.weights) and same_bits(auto.m, hand.m) and same_bits(auto.v, hand.v)
    assert same_bits(out["stats"], stats)
    assert bool((stats[:, 6] == 0).all()) and bool((stats[:, 7] == 1).all())
    # the policy the rollout kernels read holds the learner's weights
    assert np.array_equal(auto.policy.flat_weights().view(np.uint32), auto.weights.cpu().numpy().view(np.uint32))
    assert not same_bits(auto.weights, torch.from_numpy(hand.policy.flat_weights()).cuda())  # ... and they moved


def test_a_ppo_learner_continues_from_the_cloned_weights():
    import torch

    import marl_sortingenv_amd as M

    D, A = MONO
    il, _ = bc_learner(D, A, 73, "fma", n_epochs=2, batch_size=128)
    il.update(mono_demonstrations())
    cloned = il.policy
    copy = M.MlpPolicy(D, A, cloned.state_dict(), device=0, precision="f32")
    after, fresh = M.PPOLearner(cloned, n_epochs=2, batch_size=128, seed=9), M.PPOLearner(copy, n_epochs=2, batch_size=128, seed=9)
    assert same_bits(after.weights, il.weights) and same_bits(fresh.weights, il.weights)
    env = _env("mono", 64, 5, seed=13)
    data = M.FusedPolicyRollout(env, cloned, 8, seed=21).collect()
    a = after.update(data)
    b = fresh.update(data)
    torch.cuda.synchronize()
    assert same_bits(after.weights, fresh.weights) and same_bits(a["stats"], b["stats"])
    assert not same_bits(after.weights, il.weights)
    with pytest.raises(NotImplementedError):
        il.state_dict()


def test_cloning_lowers_the_loss():
    """sanity, not a score: 4 096 rows (mono, noise 0), 30 epochs at lr 1e-3"""
    import marl_sortingenv_amd as M

    data = M.DemonstrationCollector(_env("mono", 512, 50, seed=17, noise=0.0), 8).collect()
    pol = M.MlpPolicy.random_init(*MONO, seed=1, device=0)
    il = M.ImitationLearner(pol, learning_rate=1e-3, n_epochs=30, batch_size=1024, seed=3)
    stats = il.update(data)["stats"].cpu()
    first, last = float(stats[0, 1]), float(stats[-4:, 1].mean())  # the first minibatch, the last epoch's four
    print(f"bc_loss {first:.4f} -> {last:.4f}, accuracy {float(stats[0, 4]):.3f} -> {float(stats[-4:, 4].mean()):.3f}")
    assert last < first
