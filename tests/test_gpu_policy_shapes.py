"""GPU: the policy head (msep::sample_tile and the network in front of it) at every kernel shape, tie and mask edge.

  a. every k_policy_mlp<NR, F16X3> instantiation and selector edge (A = 2|3, 11|12, 24|25), D = 1, odd D and D = 32,
     against float64 torch (ids name A -> NR);
  b. row-count edges at (29, 22): tiles, blocks, a second trip of the grid-stride loop, sentinels around every output;
  c. exact ties on the constant-logit head: deterministic action == torch.argmax's first maximum, no margin excused;
  d. one-hot masks at every action index;
  e. half-only and random masks on a uniform policy: the sampled action == the float32 restatement, every row;
  f. the draws u = 0 and u = 1 - 2^-24;
  g. a mask row with no legal action: uniform over the A actions, never an action >= A;
  h. the fused rollout kernels (the three learned-policy shapes, Env_2's sorting agent, k_rollout_model) obey c and e.

References and rules: tests/policy_head_reference.py.  Actions are read to the host before anything is indexed by them."""
import math

import numpy as np
import pytest

from tests import policy_head_reference as R
from tests import policy_stream as ps

pytestmark = pytest.mark.gpu

PRECISIONS = ["f32", "f16x3"]
TIE_ACTIONS = [2, 11, 22, 32]


def _policy(D, A, w, precision):
    import marl_sortingenv_amd as M

    pol = M.MlpPolicy(D, A, w, device=0, precision=precision)
    assert pol.precision == precision
    return pol


def _obs(n, D, seed=3):
    import torch

    return (torch.rand((n, D), generator=torch.Generator().manual_seed(seed)) * 2.0 - 1.0).cuda()


def _run(pol, obs, mask, **kw):
    """forward -> host numpy arrays; mask: numpy bool [N, A] or None."""
    import torch

    dm = None if mask is None else torch.as_tensor(mask).cuda()
    out = pol.forward(obs, dm, **kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


# ---- a. every instantiation and selector edge against float64 --------------------------------------------------------
SHAPES = [(1, 1), (1, 2), (5, 3), (16, 4), (16, 8), (16, 9), (16, 11), (32, 12), (29, 22), (32, 24), (32, 25), (32, 32),
          (1, 32), (31, 32)]
CASES_A = [(D, A, "test") for D, A in SHAPES] + [(32, 32, "saturating"), (1, 32, "saturating")]


def test_shape_cases_launch_every_instantiation():
    assert {R.kernel_regs(A) for _, A, _ in CASES_A} == set(R.KERNEL_REGS)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("D,A,which", CASES_A, ids=[f"D{D}-A{A}-NR{R.kernel_regs(A)}-{w}" for D, A, w in CASES_A])
def test_policy_forward_every_shape_matches_float64(D, A, which, precision):
    """300 random rows + six edge rows.  The project's tolerances apply unchanged (LOGIT_TOL, LOGP_TOL, and
    SATURATING_F16X3_LOGIT_TOL for the split form on the saturating set); torch's own float32 error against float64 on
    the same rows is printed beside the kernel's as the yardstick (DESIGN 4.7 records both)."""
    make = R.weights if which == "test" else R.saturating_weights
    w = make(D, A, seed=D * 100 + A)
    w64 = {k: v.double() for k, v in w.items()}
    tol = R.SATURATING_F16X3_LOGIT_TOL if (which == "saturating" and precision == "f16x3") else R.LOGIT_TOL
    pol = _policy(D, A, w, precision)
    obs, mask, single = R.forward_inputs(D, A, 300)
    l32, _, v32 = R.torch_reference(w, obs, mask)
    l64, _, v64 = R.torch_reference(w64, obs.double(), mask)
    e32 = (float((l32.double() - l64).abs().max()), float((v32.double() - v64).abs().max()))
    report = {}
    try:
        R.check_forward(pol, w64, obs, mask, single, tol, report=report)
    finally:
        print(f"policy head D={D} A={A} NR={R.kernel_regs(A)} {which} {precision}: logits {report.get('logits', float('nan')):.3g} "
              f"value {report.get('value', float('nan')):.3g} (torch float32: {e32[0]:.3g} / {e32[1]:.3g}; bound {tol:g})")


# ---- b. row-count edges ----------------------------------------------------------------------------------------------
_B_CACHE = {}


def _b_case(n):
    """Inputs of n rows at (29, 22), shared by both precisions."""
    if n not in _B_CACHE:
        _B_CACHE[n] = R.forward_inputs(29, 22, n, seed=40 + n % 7, edges=False)
    return _B_CACHE[n]


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("n", [1, 31, 32, 33, 63, 64, 65, 255, 256, 257, 131072 + 33])
def test_policy_forward_row_count_edges(n, precision):
    """Tile (32), wave-pair (64) and block (256) boundaries and a second trip of the grid-stride loop (512 workgroups x
    8 waves x 32 envs = 131 072 rows per trip) against float64; every output lives inside a larger buffer whose
    neighbouring elements must survive (padding lanes of a ragged last tile write nothing)."""
    import torch

    D, A, PAD = 29, 22, 96
    w = R.weights(D, A, seed=2922)
    pol = _policy(D, A, w, precision)
    obs, mask, single = _b_case(n)
    R.check_forward(pol, {k: v.double() for k, v in w.items()}, obs, mask, single, R.LOGIT_TOL)
    band = {"action": torch.full((n + 2 * PAD,), -777, dtype=torch.int32, device="cuda"),
            "logp": torch.full((n + 2 * PAD,), 12345.0, dtype=torch.float32, device="cuda"),
            "value": torch.full((n + 2 * PAD,), 12345.0, dtype=torch.float32, device="cuda"),
            "logits": torch.full(((n + 2 * PAD) * A,), 12345.0, dtype=torch.float32, device="cuda")}
    view = {k: v[PAD:PAD + n] for k, v in band.items() if k != "logits"}
    view["logits"] = band["logits"][PAD * A:(PAD + n) * A].view(n, A)
    for det in (False, True):
        plain = pol.forward(obs.cuda(), mask.cuda(), seed=77, t=3, deterministic=det, want_logits=True)
        pol.forward(obs.cuda(), mask.cuda(), seed=77, t=3, deterministic=det, want_logits=True, out=view)
        for k, v in band.items():
            pad = PAD * (A if k == "logits" else 1)
            sent = -777 if k == "action" else 12345.0
            assert bool((v[:pad] == sent).all()) and bool((v[v.numel() - pad:] == sent).all()), (k, det)
            assert torch.equal(view[k], plain[k]), (k, det)


# ---- c. ties ---------------------------------------------------------------------------------------------------------
def _tie_cases(A):
    """(name, tied actions, actions made illegal) on a head whose other logits descend from -1 in steps of 2^-6."""
    if A == 2:
        return [("all_equal", [0, 1], []), ("pair_half0", [0, 1], []), ("lowest_masked", [0, 1], [0]),
                ("group_masked", [0], [0])]
    cases = [("all_equal", list(range(A)), []),
             ("pair_half0", [1, 9], []),
             ("pair_half1", [5, 6] if A < 15 else [5, 14], []),
             ("pair_3_4_half0_lower", [3, 4], []),
             ("pair_5_9_half1_lower", [5, 9], []),
             ("pair_4_8_half1_lower_register_too", [4, 8], []),
             ("pair_7_8", [7, 8], []),
             ("lowest_masked", [2, 6, 9], [2]),
             ("lowest_two_masked", [1, 5, 10], [1, 5]),
             ("group_masked", [3, 4], [3, 4])]
    if A > 16:
        cases += [("pair_last_registers", [A - 6, A - 1], []), ("triple_across", [19, 20, A - 1], [19])]
    return cases


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("A", TIE_ACTIONS)
def test_deterministic_ties_go_to_the_lowest_action_index(A, precision):
    """Exact ties placed by the constant-logit head: the deterministic action is torch.argmax's first maximum of the
    masked float64 logits on every row - within a half, across the halves in both orders, with the lowest member or
    the whole group masked - with the mask and with mask=None."""
    D, n = 16, 70
    obs = _obs(n, D)
    pol = None
    for name, tied, illegal in _tie_cases(A):
        bias = (-1.0 - np.arange(A) / 64.0).astype(np.float32)
        bias[tied] = np.float32(0.5)
        w = R.constant_head_weights(D, A, bias, seed=A)
        pol = _policy(D, A, w, precision) if pol is None else pol.load_weights(w)
        mask = np.ones((n, A), dtype=bool)
        mask[:, illegal] = False
        others = [a for a in range(A) if a not in tied and a not in illegal]
        if len(others) >= 2:
            mask[1::2, others[-1]] = False  # and, on every second row, an action outside the tie
        for mk in (mask, None):
            out = _run(pol, obs, mk, deterministic=True, want_logits=True)
            R.assert_constant_head(out["logits"], bias, mk)
            want = R.first_argmax(np.broadcast_to(bias.astype(np.float64), (n, A)), mk)
            bad = np.flatnonzero(out["action"] != want)
            assert bad.size == 0, (name, "masked" if mk is not None else "unmasked", int(bad[0]),
                                   int(out["action"][bad[0]]), int(want[bad[0]]))


# ---- d. one-hot masks ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("A", [1, 2, 11, 12, 22, 25, 32])
def test_one_hot_masks_at_every_action(A, precision):
    """A single legal action at every index (the last action and the last register of each half among them): taken in
    both modes, |logp| <= LOGP_TOL, every other logit exactly float32(-1e8)."""
    D, n = 16, 3 * A
    pol = _policy(D, A, R.weights(D, A, seed=7 + A), precision)
    obs = _obs(n, D)
    hot = np.arange(n) % A
    mask = np.zeros((n, A), dtype=bool)
    mask[np.arange(n), hot] = True
    for det in (False, True):
        out = _run(pol, obs, mask, seed=5, t=1, deterministic=det, want_logits=True)
        assert (out["action"] == hot).all(), det
        assert np.abs(out["logp"]).max() <= R.LOGP_TOL, det
        bits = out["logits"].view(np.uint32)
        assert (bits[~mask] == R.HUGE_NEG_BITS).all() and (bits[mask] != R.HUGE_NEG_BITS).all()


# ---- e. half-only masks, exact sampling ------------------------------------------------------------------------------
def _uniform_masks(A, n, seed):
    """name -> mask [n, A] with at least one legal action per row."""
    rng = np.random.default_rng(seed)
    half = np.array([R.half_of(a) for a in range(A)])
    rnd = rng.random((n, A)) < 0.6
    out = {}
    for h in (0, 1):
        rows = np.flatnonzero(half == h)
        if rows.size == 0:
            continue
        m = rnd & (half == h)
        m[np.arange(n), rows[rng.integers(0, rows.size, n)]] = True
        out[f"half{h}_only"] = m
    m = rnd.copy()
    m[:, 0] = True
    out["random_with_action0"] = m
    if A > 1:
        m = rnd.copy()
        m[:, 0] = False
        m[np.arange(n), rng.integers(1, A, n)] = True
        out["random_without_action0"] = m
    out["unmasked"] = None
    return out


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("A", TIE_ACTIONS)
def test_uniform_policy_samples_equal_the_float32_restatement(A, precision):
    """Bias 0 on the constant head: the sampled action equals uniform_sample_f32 on every one of 4 096 rows (no row
    excused), for masks legal only in half 0's rows (S.hi == 0), only in half 1's (S.lo == 0), random with and without
    action 0, and none; logp = -log(count)."""
    D, n, seed, t = 16, 4096, 21, 9
    bias = np.zeros(A, dtype=np.float32)
    pol = _policy(D, A, R.constant_head_weights(D, A, bias, seed=A), precision)
    obs = _obs(n, D)
    words = ps.word(seed, np.arange(n), t)
    for name, mask in _uniform_masks(A, n, seed=A).items():
        out = _run(pol, obs, mask, seed=seed, t=t, want_logits=True)
        R.assert_constant_head(out["logits"], bias, mask)
        want = R.uniform_sample_f32(words, mask, A)
        bad = np.flatnonzero(out["action"] != want)
        assert bad.size == 0, (name, bad.size, int(bad[0]), int(out["action"][bad[0]]), int(want[bad[0]]))
        count = np.full(n, A) if mask is None else mask.sum(axis=1)
        assert np.abs(out["logp"] + np.log(count)).max() <= R.LOGP_TOL, name
        det = _run(pol, obs, mask, deterministic=True)["action"]
        assert (det == (0 if mask is None else np.argmax(mask, axis=1))).all(), name


# ---- f. extreme draws ------------------------------------------------------------------------------------------------
def _end_masks(A):
    order = R.register_order(A)
    masks = {"all_legal": np.ones(A, dtype=bool)}
    ends = np.ones(A, dtype=bool)
    for h in (0, 1):
        rows = [a for a in order if R.half_of(a) == h]
        if len(rows) >= 3:
            ends[[rows[0], rows[-1]]] = False
        elif len(rows) == 2:
            ends[rows[0]] = False
    masks["ends_illegal"] = ends
    for h in (0, 1):
        rows = [a for a in order if R.half_of(a) == h]
        if len(rows) >= 3:
            m = np.zeros(A, dtype=bool)
            m[rows[1:-1]] = True
            masks[f"half{h}_only_ends_illegal"] = m
    return masks


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("A", TIE_ACTIONS)
def test_extreme_draws_pick_the_first_and_last_legal_register(A, precision):
    """u = 0 picks the first legal register in register order (leading illegal registers have running sum 0, which
    does not exceed 0); u = 1 - 2^-24 picks the last one (the guard keeps the target below the mass) - at the committed
    env indices, placed on row 7 of 64 through index_offset; all 64 rows equal the float32 restatement."""
    D, n = 16, 64
    bias = np.zeros(A, dtype=np.float32)
    pol = _policy(D, A, R.constant_head_weights(D, A, bias, seed=A), precision)
    obs = _obs(n, D)
    for idx, top in [(i, False) for i in R.U_ZERO_INDICES] + [(i, True) for i in R.U_MAX_INDICES]:
        words = ps.word(R.EXTREME_SEED, idx - 7 + np.arange(n), R.EXTREME_T)
        assert int(words[7]) >> 8 == (0xFFFFFF if top else 0)
        for name, row in _end_masks(A).items():
            mask = np.broadcast_to(row, (n, A)).copy()
            out = _run(pol, obs, mask, seed=R.EXTREME_SEED, t=R.EXTREME_T, index_offset=idx - 7, want_logits=True)
            R.assert_constant_head(out["logits"], bias, mask)
            want = R.last_legal_register(row, A) if top else R.first_legal_register(row, A)
            assert int(out["action"][7]) == want, (name, idx, int(out["action"][7]), want)
            assert (out["action"] == R.uniform_sample_f32(words, mask, A)).all(), (name, idx)
            assert abs(float(out["logp"][7]) + math.log(int(row.sum()))) <= R.LOGP_TOL


# ---- g. no legal action ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("A", [1, 2, 3, 11, 22, 25, 32])
def test_mask_row_without_a_legal_action_is_uniform_over_the_actions(A, precision):
    """sb3_contrib's MaskableCategorical turns an all-zero mask row into A logits of -1e8: the uniform distribution.
    Registers that hold no action (for A = 22, 2 of the 24 the kernel walks) must carry no mass: over 8 192 such rows
    every one of the A actions occurs and nothing else, logp = -log A, and the deterministic action is 0 - whatever
    the network's own logits are.  Rows with legal actions in the same tiles are untouched."""
    D, n = 16, 8192
    pol = _policy(D, A, R.weights(D, A, seed=50 + A), precision)
    obs = _obs(n + 64, D)
    mask = np.zeros((n + 64, A), dtype=bool)
    mask[n:, 0] = True  # the last two tiles: rows with one legal action
    out = _run(pol, obs, mask, seed=13, t=2, want_logits=True)
    act = out["action"]
    assert act.min() >= 0 and act.max() < A, (int(act.min()), int(act.max()))
    assert (np.bincount(act[:n], minlength=A) > 0).all()
    assert np.abs(out["logp"][:n] + math.log(A)).max() <= R.LOGP_TOL, float(np.abs(out["logp"][:n] + math.log(A)).max())
    assert (out["logits"].view(np.uint32)[:n] == R.HUGE_NEG_BITS).all()
    assert (act[n:] == 0).all() and np.abs(out["logp"][n:]).max() <= R.LOGP_TOL
    # uniform: 4 sigma of a binomial count per action
    freq = np.bincount(act[:n], minlength=A) / n
    assert np.abs(freq - 1.0 / A).max() <= 4.0 * math.sqrt((1.0 / A) * (1.0 - 1.0 / A) / n) + 1e-12
    det = _run(pol, obs, mask, deterministic=True)["action"]
    assert (det == 0).all()


# ---- h. the fused kernels --------------------------------------------------------------------------------------------
def _zero_head(D, A, seed=0):
    import marl_sortingenv_amd as M

    pol = M.MlpPolicy(D, A, R.constant_head_weights(D, A, np.zeros(A, dtype=np.float32), seed=seed), device=0, precision="f16x3")
    assert pol.precision == "f16x3"
    return pol


@pytest.mark.parametrize("pipeline", [0, 1, 2])
@pytest.mark.parametrize("kind", ["mono", "press", "sort"])
def test_fused_policy_rollout_obeys_the_head_rules(kind, pipeline):
    """A zero-head policy (every logit 0) inside the three learned-policy rollout shapes: deterministic actions are
    the first legal action of the recorded mask, sampled actions equal uniform_sample_f32 of the env's word for that
    step, on every row; unmasked: action 0, and uniform over all A."""
    import marl_sortingenv_amd as M

    n, K, seed = 97, 12, 6
    env = M.BatchedSortingEnv(kind=kind, num_envs=n, device=0, base_seed=19, max_steps=5, noise_sorting=0.05,
                              balesize=200, rollout_pipeline=pipeline)
    A = env.num_actions
    pol = _zero_head(env.obs_dim, A, seed=3)
    fused = M.FusedPolicyRollout(env, pol, K, seed=seed)
    idx = env.index_offset + np.arange(n)
    for det, masking in ((True, True), (False, True), (True, False), (False, False), (False, True)):
        t0 = env.policy_step
        b = fused.collect(deterministic=det, use_action_masking=masking)
        act, masks = b["actions"].cpu().numpy(), b["action_masks"].cpu().numpy() != 0
        logp = b["log_probs"].cpu().numpy()
        assert env.policy_step == t0 + K and masks.any(axis=2).all()
        for k in range(K):
            mk = masks[k] if masking else None
            if det:
                want = np.argmax(masks[k], axis=1) if masking else np.zeros(n, dtype=np.int64)
            else:
                want = R.uniform_sample_f32(ps.word(seed, idx, t0 + k), mk, A)
            bad = np.flatnonzero(act[k] != want)
            assert bad.size == 0, (det, masking, k, int(bad[0]), int(act[k][bad[0]]), int(want[bad[0]]))
            count = masks[k].sum(axis=1) if masking else np.full(n, A)
            assert np.abs(logp[k] + np.log(count)).max() <= R.LOGP_TOL
    assert env.error_count() == 0


@pytest.mark.parametrize("pipeline", [0, 2])
def test_fused_rollout_zero_head_sorting_agent_equals_sort_mode_zero(pipeline):
    """Env_2 with a zero-head sorting agent (both logits 0: the tie goes to action 0) records the rows of sort_mode all
    zero."""
    import torch

    import marl_sortingenv_amd as M

    n, K = 97, 12
    kw = dict(kind="press", num_envs=n, device=0, base_seed=23, max_steps=5, noise_sorting=0.05, balesize=200,
              rollout_pipeline=pipeline)
    a, b = M.BatchedSortingEnv(**kw), M.BatchedSortingEnv(**kw)
    pol = M.MlpPolicy(16, 11, R.weights(16, 11, seed=41), device=0)
    fa = M.FusedPolicyRollout(a, pol, K, seed=8, sort_policy=_zero_head(13, 2, seed=5))
    fb = M.FusedPolicyRollout(b, pol, K, seed=8, sort_mode=torch.zeros(n, dtype=torch.int32))
    for it in range(2):
        x, y = fa.collect(), fb.collect()
        for key in x:
            assert torch.equal(x[key], y[key]), (it, key)
    for sa, sb in zip(a.get_state(), b.get_state()):
        assert torch.equal(sa, sb)


@pytest.mark.parametrize("masked", [True, False], ids=["press_agent_masked", "press_agent_unmasked"])
def test_fused_model_rollout_zero_head_agents(masked):
    """k_rollout_model with zero-head agents: the sorting part of every action is 0; the pressing part is the first
    legal entry of the press mask the agent is shown (the first 11 entries of the mask of the state before the step),
    or 0 when it is shown none."""
    import torch

    import marl_sortingenv_amd as M

    n, K = 97, 12
    env = M.BatchedSortingEnv(kind="mono", num_envs=n, device=0, base_seed=31, max_steps=5, noise_sorting=0.05,
                              balesize=200, auto_reset=True)
    sort_ag, press_ag = _zero_head(13, 2, seed=1), _zero_head(16, 11, seed=2)
    env.refresh_outputs()
    before = env.mask.clone()
    buf = env.rollout(K, policy="model", sort_agent=sort_ag, press_agent=press_ag, press_agent_maskable=masked)
    act = buf["actions"].cpu().numpy()
    shown = torch.cat([before[None], buf["mask"][:-1]]).cpu().numpy()[:, :, :11] != 0
    assert ((act >= 0) & (act < 22)).all() and (act // 11 == 0).all()
    assert shown.any(axis=2).all()
    want = np.argmax(shown, axis=2) if masked else np.zeros_like(act)
    assert (act % 11 == want).all()
    assert int(buf["done"].sum()) >= 2 * n and env.error_count() == 0
